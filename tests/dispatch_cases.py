"""Small scenes that reach the size-selected kernels of the fused path, and the dispatch rule restated (design/19_dispatch_thresholds.md).

Which kernel a launch runs is decided from T = tiles / workgroups (Fused, CameraItems, launch_stream at the end of
csrc/kernels_bal.inc; the thresholds are the named constants of csrc/common.h, parsed here — never repeated).  solver.hip launches
min(CUs, ceil(tiles / 8)) workgroups, so a scene of a few hundred tiles always has T <= 8 — unless CERES_HIP_FUSED_GRID caps the
workgroups; and plan.cc cuts the camera-major pass's items at n_obs / kCamItemSpread observations (64 on a small scene) unless
CERES_HIP_CAM_CHUNK_MIN raises that.  Both switches are read per handle, at set_structure: tests set them with monkeypatch.setenv.

tests/test_dispatch_cases_cpu.py holds every scene to the threshold it is meant for, from host-only data; tests/test_gpu_dispatch.py
runs them.  numpy and the package's generators only."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceres-solver_amd", "csrc")
DEVICE_CUS = 256            # compute units of an MI355X: the workgroups of an uncapped launch
CAM_CHUNK_MIN = 512         # CERES_HIP_CAM_CHUNK_MIN of the scenes whose items are to be full length (= kCamChunk)


@functools.lru_cache(maxsize=None)
def constants():
    """The integer constants of csrc/common.h by name."""
    with open(os.path.join(CSRC, "common.h")) as f:
        text = f.read()
    k = {name: int(v) for name, v in re.findall(r"constexpr\s+(?:int|size_t)\s+(\w+)\s*=\s*(\d+)\s*;", text)}
    k["kLdsBytesPerCu"] = int(re.search(r"kLdsBytesPerCu\s*=\s*(\d+)\s*\*\s*1024", text).group(1)) * 1024
    for name in ("kTile", "kCamChunk", "kPipelineMinTilesPerWg", "kStagedXMinTilesPerWg", "kCamItemLaneMinMean", "kCamItemSpread",
                 "kNonTemporalTileMiB"):
        assert name in k, name
    return k


@functools.lru_cache(maxsize=None)
def compiled_shapes():
    """The shapes kernels_bal_common.hip declares launchers for: 'f6_s0', 'e4_f6_s0', 'r4_e4_f2_s0', ... in its order."""
    with open(os.path.join(CSRC, "kernels_bal_common.hip")) as f:
        return tuple(re.findall(r"^const BalOps\* BalOps_bal_(\w+)\(\);", f.read(), flags=re.M))


def shape_of(name):
    """(nr, ne, nf, ns) of a shape name."""
    m = re.fullmatch(r"(?:r(\d+)_)?(?:e(\d+)_)?f(\d+)_s(\d+)", name)
    return int(m.group(1) or 2), int(m.group(2) or 3), int(m.group(3)), int(m.group(4))


# what structured_bal needs to produce each strip shape: shared blocks that fill the compiled strip width (or round up to it: 5 + 2),
# libmv's locked first camera on the 6-wide poses.  No 3-wide shared block: CGNR would read it as a point and leave the fused path.
STRIPS = {"f6_s4": dict(shared_widths=(4,), locked_cameras=(0,)), "f6_s8": dict(shared_widths=(8,), locked_cameras=(0,)),
          "f9_s4": dict(shared_widths=(2, 2), shared_first=False), "f9_s8": dict(shared_widths=(5, 2))}


def shape_kwargs(name):
    nr, ne, nf, ns = shape_of(name)
    kw = dict(camera_width=nf, point_width=ne, row_height=nr)
    if ns:
        kw.update(STRIPS[name])
    return kw


def pipelined(name):
    """The shapes with software-pipelined kernels: 2-high rows on 3-wide points (CERES_HIP_PIPELINED, kernels_bal.inc)."""
    nr, ne, _, _ = shape_of(name)
    return nr == 2 and ne == 3


PIPELINED_SHAPES = tuple(n for n in compiled_shapes() if pipelined(n))
OTHER_SHAPES = tuple(n for n in compiled_shapes() if not pipelined(n))


def cgnr_fused(name):
    """Whether CGNR (no elimination order: "points" are whatever is 3 wide) reads this Schur-ordered Jacobian as a fused shape of its
    own.  A 3-wide camera or shared block cannot be told from a point: the generic kernels (tests/test_gpu_shapes.py)."""
    nr, ne, nf, ns = shape_of(name)
    return pipelined(name) and nf != 3 and 3 not in STRIPS.get(name, {}).get("shared_widths", ())


# ---- the dispatch rule, restated ----------------------------------------------------------------------------------------------------
def grid(n_tiles, grid_cap=None, cus=DEVICE_CUS):
    """Workgroups of the fused launches with every camera's accumulator in LDS (solver.hip: fused_grid)."""
    g = cus if not grid_cap else min(cus, grid_cap)
    return max(1, min(g, (n_tiles + 7) // 8))


def fused_kernel(n_tiles, grid_cap, name, cus=DEVICE_CUS):
    """'512' | 'pipelined' | '1024': what S.x, JtJx and the power-series operator run on (operator calls: no CG tail)."""
    if n_tiles < constants()["kPipelineMinTilesPerWg"] * grid(n_tiles, grid_cap, cus):
        return "512"
    return "pipelined" if pipelined(name) else "1024"


def x_staged(n_tiles, grid_cap, cus=DEVICE_CUS):
    """Whether a workgroup stages x in LDS: the staged cameras' rows in the streaming kernels, all of it in back-substitution."""
    return n_tiles >= constants()["kStagedXMinTilesPerWg"] * grid(n_tiles, grid_cap, cus)


def camera_items(degrees, n_obs, chunk_min=None):
    """The items plan.cc cuts the cameras' lists into: (camera, length) arrays; a camera without observations has one empty item."""
    k = constants()
    chunk = max(chunk_min or k["kTile"], min(k["kCamChunk"], (n_obs // k["kCamItemSpread"] + k["kTile"] - 1) // k["kTile"] * k["kTile"]))
    cams, lens = [], []
    for c, d in enumerate(np.asarray(degrees, dtype=np.int64)):
        n = max(1, -(-int(d) // chunk))
        cams += [c] * n
        lens += [min(chunk, int(d) - i * chunk) for i in range(n)]
    return np.asarray(cams), np.asarray(lens)


def camera_item_kernel(degrees, n_obs, name, chunk_min=None):
    """'lane' (bal_camera_items_kernel, a lane per observation) | 'mfma' (bal_camera_items_mfma_kernel: 2-high rows, short items)."""
    _, lens = camera_items(degrees, n_obs, chunk_min)
    mfma = shape_of(name)[0] == 2 and int(np.sum(degrees)) < constants()["kCamItemLaneMinMean"] * len(lens)
    return "mfma" if mfma else "lane"


def camera_degrees(hs, p):
    """(observations with a camera cell per camera — a locked camera has none —, tiles) from the host-side plan set_structure builds
    (debug_staged_x_plan: points renumbered; debug_plan packs the caller's point order, into a few tiles more)."""
    assert hs.debug_plan(p.bs, p.num_eliminate_blocks)["eligible"]
    sx = hs.debug_staged_x_plan(p.bs, p.num_eliminate_blocks)
    word = sx["slot_word"][sx["slot_word"] >= 0]
    return np.bincount(word & ((1 << constants()["kSlotCamBits"]) - 1), minlength=sx["n_cameras"]), int(sx["n_tiles"])


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------
FEW_CAMERAS, FEW_POINTS, FEW_RARE = 8, 3640, 40
FEW_GRID_CAPS = (1, 3)


@functools.lru_cache(maxsize=None)
def few_cameras_visibility():
    """8 cameras, 3640 points of 4 .. 7 observations by the first seven cameras (popularity ~ (c + 1)^-0.5), the eighth camera on 40
    points only: 19 968 observations in 319 tiles (7 mod 8 and mod 24: the waves of a workgroup take unequal numbers of tiles under
    either cap), some 2 800 per camera — five or six items of 512 each and a ragged last one — and one camera of a single item shorter
    than a wavefront.  (point_of_obs, cam_of_obs), sorted by point, then camera."""
    rng = np.random.default_rng(1907)
    k = rng.integers(4, 8, size=FEW_POINTS)
    w = np.arange(1, FEW_CAMERAS, dtype=np.float64) ** -0.5
    w /= w.sum()
    cams = [rng.choice(FEW_CAMERAS - 1, size=int(n), replace=False, p=w) for n in k]
    rare = np.sort(rng.choice(FEW_POINTS, size=FEW_RARE, replace=False))
    pt = np.concatenate([np.repeat(np.arange(FEW_POINTS, dtype=np.int64), k), rare])
    cam = np.concatenate(cams + [np.full(FEW_RARE, FEW_CAMERAS - 1)]).astype(np.int64)
    order = np.lexsort((cam, pt))
    return pt[order], cam[order]


def _damp_empty_columns(p):
    """A locked camera's columns are empty: the generator's D there is sqrt(1e-6 / 1e4), the camera's block D^2 = 1e-10 and its
    inverse 1e10 — in a norm over all inverted blocks that one exact block would hide every other.  D = 1 on such columns."""
    if p.D is not None:
        p.D = np.where(p.D <= 1.0001e-5, 1.0, p.D)
    return p


def few_cameras(problems, name, layout="schur", with_values=True, seed=11):
    pt, cam = few_cameras_visibility()
    return _damp_empty_columns(problems.structured_bal(FEW_CAMERAS, FEW_POINTS, pt, cam, layout=layout, seed=seed, with_values=with_values,
                                                       **shape_kwargs(name)))


LDS_GRID_CAP = 2
LDS_POINTS = 5040


def lds_filling_cameras(name):
    """As many cameras as leave the staged x a handful of rows beside the accumulators (plan.cc reserves 1 KiB for static arrays):
    2 250 for 9-wide cameras, as tests/test_gpu_fullsize.py::test_popular_cameras_x_in_lds_at_the_edges_of_the_budget."""
    _, _, nf, ns = shape_of(name)
    return (constants()["kLdsBytesPerCu"] - 1024) // (8 * nf) - 11 - -(-ns // nf)


@functools.lru_cache(maxsize=None)
def lds_filling_visibility(n_cams):
    """5040 points of 2 .. 6 observations.  Observation i is camera i mod n_cams — every camera is seen, also where there are more
    cameras than half the observations; a camera nobody sees has the block D^2 = 1e-10, whose inverse of 1e10 would drown every other
    camera's in a norm over all blocks — and half of the observations past the first sweep move to one of 64 popular cameras
    (~ (c + 1)^-0.6) unless their point has that camera already: the staged rows are those, and almost every tile has slots of both kinds."""
    rng = np.random.default_rng(23)
    k = rng.integers(2, 7, size=LDS_POINTS)
    pt = np.repeat(np.arange(LDS_POINTS, dtype=np.int64), k)
    n_obs = pt.shape[0]
    base = np.arange(n_obs, dtype=np.int64) % n_cams
    w = np.arange(1, 65, dtype=np.float64) ** -0.6
    moved = (np.arange(n_obs) >= n_cams) & (rng.random(n_obs) < 0.5)
    cam = np.where(moved, rng.choice(64, size=n_obs, p=w / w.sum()), base)
    while True:
        key, inverse, count = np.unique(pt * n_cams + cam, return_inverse=True, return_counts=True)
        back = moved & (count[inverse] > 1)
        if not back.any():
            break
        cam[back], moved[back] = base[back], False
    order = np.lexsort((cam, pt))
    return pt[order], cam[order]


def lds_filling(problems, name, layout="schur", with_values=True, seed=23):
    n_cams = lds_filling_cameras(name)
    pt, cam = lds_filling_visibility(n_cams)
    p = _damp_empty_columns(problems.structured_bal(n_cams, LDS_POINTS, pt, cam, layout=layout, seed=seed, with_values=with_values,
                                                    **shape_kwargs(name)))
    if with_values:
        # Thousands of cameras share 20 000 observations: most have about as many rows as columns, some fewer, and their blocks are
        # as ill-conditioned as the damping lets them be.  At the generator's trust-region radius of 1e4 (condition numbers up to 1e7)
        # two float64 inverses of the same blocks — numpy's LU and Cholesky — differ by 0.7 .. 1.1e-12 in the norm the tests use, the
        # bound itself; at a radius of 1e2 by 1.5e-14 at most (design/19_dispatch_thresholds.md).
        p.D = p.D * 10.0
    return p


BOUNDARY_SHAPE, BOUNDARY_GRID_CAP = "f6_s0", 1


def boundary_tiles():
    k = constants()
    return (k["kPipelineMinTilesPerWg"] - 1, k["kPipelineMinTilesPerWg"], k["kStagedXMinTilesPerWg"] - 1, k["kStagedXMinTilesPerWg"])


@functools.lru_cache(maxsize=None)
def _boundary_visibility():
    rng = np.random.default_rng(31)
    n_c, n_p, n_obs = 30, 2000, 9000
    k = np.clip(rng.geometric(1.0 / (1.0 + n_obs / n_p - 2), size=n_p) + 1, 2, n_c)
    pt = np.repeat(np.arange(n_p, dtype=np.int64), k)
    w = np.arange(1, n_c + 1, dtype=np.float64) ** -0.5
    cam = np.concatenate([rng.choice(n_c, size=int(n), replace=False, p=w / w.sum()) for n in k]).astype(np.int64)
    order = np.lexsort((cam, pt))
    return n_c, pt[order], cam[order], np.concatenate([[0], np.cumsum(k)])


@functools.lru_cache(maxsize=None)
def _boundary_points(hs, problems, n_tiles):
    """The number of leading points of the boundary visibility whose scene packs into exactly n_tiles tiles."""
    n_c, pt, cam, ptr = _boundary_visibility()
    kw = shape_kwargs(BOUNDARY_SHAPE)

    def tiles(n):
        p = problems.structured_bal(n_c, n, pt[:ptr[n]], cam[:ptr[n]], with_values=False, **kw)
        return int(hs.debug_staged_x_plan(p.bs, p.num_eliminate_blocks)["n_tiles"])
    lo, hi = 1, len(ptr) - 1
    assert tiles(hi) > n_tiles
    while lo < hi:   # the fewest points that need n_tiles tiles (a point adds at most a tile)
        mid = (lo + hi) // 2
        if tiles(mid) >= n_tiles:
            hi = mid
        else:
            lo = mid + 1
    for n in range(lo, lo + 64):   # (the packer renumbers points: the count need not be monotone in n)
        if tiles(n) == n_tiles:
            return n
    raise AssertionError(f"no prefix of the boundary scene packs into {n_tiles} tiles")


def boundary(hs, problems, n_tiles, seed=37):
    n_c, pt, cam, ptr = _boundary_visibility()
    n = _boundary_points(hs, problems, n_tiles)
    return problems.structured_bal(n_c, n, pt[:ptr[n]], cam[:ptr[n]], seed=seed, **shape_kwargs(BOUNDARY_SHAPE))


# every point of the libmv visibility has more than 64 observations: whole tiles, taken in cooperative rounds by the streaming kernels
LONG_POINT_SHAPES = {"f6_s0": {}, "f10_s0": {}, "f6_s8": dict(locked_cameras=(0,))}


def long_points(problems, name, with_values=True, seed=3):
    n_c, n_p, cam_of, pt_of = problems.libmv_visibility(2)
    order = np.lexsort((cam_of, pt_of))
    kw = dict(shape_kwargs(name), **LONG_POINT_SHAPES[name])
    return _damp_empty_columns(problems.structured_bal(n_c, n_p, pt_of[order], cam_of[order], seed=seed, with_values=with_values, **kw))


def long_points_grid_cap(n_tiles):
    """The largest cap that still leaves kPipelineMinTilesPerWg tiles per workgroup."""
    return max(1, n_tiles // constants()["kPipelineMinTilesPerWg"])


LONG_POINTS_STAGED_CAP = 2   # ... and one under which x is staged as well (rounds that read x from LDS)
