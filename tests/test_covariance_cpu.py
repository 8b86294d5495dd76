"""The covariance restatement (tests/covariance_reference.py) held to things that do not depend on it — the reference's own known
answers and its two routes against each other — the conditions the scenes of tests/covariance_cases.py must meet for the rank rule
(ceres_hip_covariance_options.min_scaled_pivot = 1e-8) to be a property of the inputs, and what ceres_hip_bal_covariance answers
without a device."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import covariance_cases as CC
import covariance_reference as CR
from conftest import ROOT, pkg

KNOWN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "covariance_known_answers.json")


def known_cases():
    d = json.load(open(KNOWN))
    sizes = d["block_sizes"]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for c in d["cases"]:
        yield d, c, sizes, starts


@pytest.mark.parametrize("eliminated", [[2], [0], [1]], ids=lambda e: "E=" + "".join("xyz"[i] for i in e))
def test_both_routes_reproduce_the_known_answers(eliminated):
    """CovarianceTest.NormalBehavior and ConstantParameterBlock at the reference's own tolerance, every block pair in both orders; route
    (b) with each block in turn as the eliminated one."""
    for d, c, sizes, starts in known_cases():
        J = np.array(d["jacobian"], dtype=np.float64)
        expected = np.array(c["expected_covariance"], dtype=np.float64)
        free = [b for b in range(len(sizes)) if b not in c["constant_blocks"]]
        elim = [b for b in eliminated if b in free]
        order = elim + [b for b in free if b not in elim]
        cols = np.concatenate([np.arange(starts[b], starts[b + 1]) for b in order])
        Jr = J[:, cols]
        a = CR.dense_covariance(Jr)
        b = CR.schur_covariance(Jr, [sizes[b] for b in elim])
        assert b["cov"] is not None and b["min_point_pivot"] > 1e-4 and b["min_schur_pivot"] > 1e-4
        for got in (a, b["cov"]):
            full = np.zeros_like(expected)
            full[np.ix_(cols, cols)] = got
            for p in range(len(sizes)):
                for q in range(len(sizes)):
                    rp, rq = slice(starts[p], starts[p + 1]), slice(starts[q], starts[q + 1])
                    diff = np.linalg.norm(expected[rp, rq] - full[rp, rq]) / (sizes[p] * sizes[q])
                    assert diff <= d["tolerance"], (c["name"], p, q, diff)


@pytest.mark.parametrize("name", CC.SUCCESS)
def test_the_routes_agree_and_the_pivots_are_large(oracle, name):
    """Routes (a) and (b) agree on every requested block, and the smallest scaled pivot of a success case is >= 1e-4: ten thousand
    times the default limit."""
    hs = pkg.hip_solver
    c = CC.case(oracle, name)
    layout, J, a, b = CC.reference_results(oracle, hs, name)
    assert J.shape[1] == layout.n
    print(f"{name}: n = {layout.n} (n_f = {layout.cw * layout.nfc}), min_point_pivot = {b['min_point_pivot']:.3e}, min_schur_pivot = {b['min_schur_pivot']:.3e}")
    assert b["cov"] is not None
    assert min(b["min_point_pivot"], b["min_schur_pivot"]) >= 1e-4
    scales = layout.scales(np.diag(a), c.pairs)
    dev = CR.correlation_deviation(layout.blocks(b["cov"], c.pairs), layout.blocks(a, c.pairs), scales)
    print(f"{name}: route (a) against route (b): {dev:.3e}")
    assert dev <= 2e-9, dev   # (float64 on unit-diagonal matrices whose pivots are >= 1e-4: n eps / pivot = 1e3 x 2.2e-16 / 1e-4 = 2e-9 at the very worst)
    # a pair with a constant block is zeros, and (b, a) is the transpose of (a, b)
    blocks = layout.blocks(b["cov"], c.pairs)
    for (p, q), blk in zip(c.pairs, blocks):
        if layout.columns(int(p)) is None or layout.columns(int(q)) is None:
            assert not blk.any()
        assert blk.shape == (layout.size(int(p)), layout.size(int(q)))


def test_scene_shapes():
    """The sizes the scenes exist for: 54 (under one 128-column panel), 270 and 279 (two panels and a remainder), 576, and 640 (five panels)."""
    import conftest
    oracle = conftest.entry.load_oracle()
    hs = pkg.hip_solver
    want = {"A-cameras01": 54, "B-cameras01": 270, "B-camera0-point0": 279, "B-cameras01-points3": 270, "C-manifold": 576, "C-angle_axis-huber": 576,
            "C-quaternion": 640}
    for name, nf in want.items():
        layout = CC.reference_results(oracle, hs, name)[0]
        assert layout.cw * layout.nfc == nf, (name, layout.cw * layout.nfc)
    c = CC.case(oracle, "C-manifold")
    counts = np.bincount(c.scene[3], minlength=c.npts)
    assert [int(counts[q]) for q in (0, 1, 2, 3, CC.TWO_OBSERVATION_POINT)] == [32, 33, 64, 65, 2]
    b = CC.case(oracle, "B-cameras01-points3")
    cam, pt = b.scene[2], b.scene[3]
    assert np.any(b.cp[pt] & b.cc[cam]) and np.any(b.cp[pt] & ~b.cc[cam])   # a removed row, and rows without an E cell
    assert len(CC.case(oracle, "A-cameras01").pairs) == (8 + 40) ** 2


@pytest.mark.parametrize("name", CC.FAILURE)
def test_failure_cases_have_vanishing_pivots(oracle, name):
    """The smallest pivot of the factorisation that fails is <= 1e-10: a hundred times under the default limit."""
    hs = pkg.hip_solver
    c = CC.case(oracle, name)
    layout, J, a, b = CC.reference_results(oracle, hs, name)
    print(f"{name}: n_f = {layout.cw * layout.nfc}, min_point_pivot = {b['min_point_pivot']:.3e}, min_schur_pivot = {b['min_schur_pivot']:.3e}")
    assert b["cov"] is None
    if c.stage == "point":
        assert b["min_point_pivot"] <= 1e-10 and b["min_schur_pivot"] == -1.0
    else:
        assert b["min_point_pivot"] >= 1e-4 and b["min_schur_pivot"] <= 1e-10


def test_refusals_without_a_device():
    """A NULL handle answers CERES_HIP_E_INVALID before any device call, with its message in ceres_hip_bal_last_error(NULL); the default
    options are the documented ones."""
    hs = pkg.hip_solver
    lib = hs.load_library()
    S = hs.CCovarianceSummary()
    x = np.zeros(4)
    a = np.zeros(1, dtype=np.int32)
    out = np.full(9, 7.0)
    rc = lib.ceres_hip_bal_covariance(None, None, hs._p(x), 1, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), hs._p(out), ctypes.byref(S))
    assert rc == -1
    assert b"NULL problem handle" in lib.ceres_hip_bal_last_error(None)
    assert np.all(out == 7.0)
    assert lib.ceres_hip_bal_covariance(None, None, None, 0, None, None, None, None) == -1
    o = hs.CCovarianceOptions(apply_loss_function=0, reserved=5, min_scaled_pivot=3.0)
    lib.ceres_hip_covariance_default_options(ctypes.byref(o))
    assert (o.apply_loss_function, o.reserved, o.min_scaled_pivot) == (1, 0, 1e-8)
    lib.ceres_hip_covariance_default_options(None)   # (returns)


def test_struct_layouts_match_the_header(tmp_path):
    """The two covariance structs of the ctypes binding have the size and the field offsets the C compiler gives include/ceres_hip.h (the
    method of test_abi_cpu.test_struct_layouts_match_the_header)."""
    hs = pkg.hip_solver
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = {"ceres_hip_covariance_options": hs.CCovarianceOptions, "ceres_hip_covariance_summary": hs.CCovarianceSummary}
    lines = ['#include "ceres_hip.h"', "#include <stddef.h>", "#include <stdio.h>", "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {fname}));')
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().splitlines()
    assert len(out) == len(pairs)
    for line, (cname, cls) in zip(out, pairs.items()):
        got = line.split()
        assert got[0] == cname
        want = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
        assert [int(v) for v in got[1:]] == want, cname
