"""A slice of the randomised parity campaign (tools/fuzz_parity.py) inside the GPU suite: sixty BAL-like structures drawn at random —
camera counts around the wavefront and LDS limits, track lengths around the tile size, single-observation points, every compiled
width, shared blocks, locked cameras, rows without a point cell — each through every operator of both solvers, fixed-count solves and
an LM step against the oracle.  (The campaign found the leftover-row kernels missing for cameras 5 and 7 wide; 860 further cases: the
worst deviation 1.5e-14.)"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuzz(hip):
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("first", [0, 20, 40])
def test_random_structures_against_the_oracle(fuzz, first):
    # Every case must pass on its first run.  (A retry once hid case 17 here: errors of 2e-2, not rounding; tests/test_gpu_schur_state.py
    # checks that case, on fresh handles after a dirty allocator and with poisoned allocations, against a numpy restatement.)
    for seed in range(first, first + 20):
        r = fuzz.run_case(seed)
        assert r["ok"], (seed, r["bad"], r)
