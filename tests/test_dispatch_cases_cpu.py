"""The scenes of tests/dispatch_cases.py reach the kernels they are meant for — from host-only data (the tile plan, the staged-x plan,
camera degrees), so that a scene which drifts below a threshold fails here instead of quietly testing the small-problem kernels once
more on the GPU.  Prints the counts (pytest -s)."""
import numpy as np
import pytest

import dispatch_cases as D


@pytest.fixture(scope="module")
def hs():
    import __graft_entry__ as entry
    hs = entry.load_package().hip_solver
    hs.load_library()
    return hs


def test_thresholds_are_named_in_the_header_and_used_by_the_dispatch():
    k = D.constants()
    assert 0 < k["kPipelineMinTilesPerWg"] < k["kStagedXMinTilesPerWg"]
    assert k["kTile"] <= k["kCamItemLaneMinMean"] <= k["kCamChunk"] == D.CAM_CHUNK_MIN
    with open(D.os.path.join(D.CSRC, "kernels_bal.inc")) as f:
        inc = f.read()
    tail = inc[inc.index("static hipError_t launch_stream("):]
    for name in ("kPipelineMinTilesPerWg", "kStagedXMinTilesPerWg", "kCamItemLaneMinMean", "kNonTemporalTileMiB"):
        assert name in tail, name
    with open(D.os.path.join(D.CSRC, "plan.cc")) as f:
        assert "kCamItemSpread" in f.read()


def test_every_compiled_shape_is_in_the_parametrisation():
    """common.h's BalShapeCompiled, the launcher table of kernels_bal_common.hip and the two shape lists of tests/test_gpu_dispatch.py
    are one list: a shape added later cannot be forgotten."""
    shapes = D.compiled_shapes()
    assert len(shapes) == len(set(shapes)) == 31
    assert sorted(D.PIPELINED_SHAPES + D.OTHER_SHAPES) == sorted(shapes)
    assert len(D.PIPELINED_SHAPES) == 13 and len(D.OTHER_SHAPES) == 18
    # BalShapeCompiled, restated from common.h's text: every (nr, ne, nf, ns) it accepts has a launcher and the other way round
    def compiled(nr, ne, nf, ns):
        if nr == 3:
            return (ne, nf, ns) == (3, 3, 0)
        if nr == 4:
            return ne == 4 and ns == 0 and nf in (2, 3, 4)
        if nr != 2:
            return False
        if ne == 2:
            return ns == 0 and nf in (2, 3, 4, 6, 9)
        if ne == 4:
            return ns == 0 and 2 <= nf <= 10
        if ne != 3:
            return False
        return 2 <= nf <= 10 if ns == 0 else (nf in (6, 9) and ns in (4, 8))
    want = {(nr, ne, nf, ns) for nr in range(1, 6) for ne in range(1, 6) for nf in range(1, 12) for ns in (0, 4, 8) if compiled(nr, ne, nf, ns)}
    assert {D.shape_of(n) for n in shapes} == want
    import test_gpu_dispatch as T
    assert sorted(T.PIPELINED_SHAPES) == sorted(D.PIPELINED_SHAPES) and sorted(T.OTHER_SHAPES) == sorted(D.OTHER_SHAPES)
    assert sorted(T.ALL_SHAPES) == sorted(shapes)


def test_the_restated_rule_at_its_edges():
    k = D.constants()
    lo, hi = k["kPipelineMinTilesPerWg"], k["kStagedXMinTilesPerWg"]
    assert D.grid(319, None) == 40 and D.grid(319, 3) == 3 and D.grid(5, 3) == 1 and D.grid(100000, None) == D.DEVICE_CUS
    assert D.fused_kernel(lo - 1, 1, "f6_s0") == "512" and D.fused_kernel(lo, 1, "f6_s0") == "pipelined"
    assert D.fused_kernel(3 * lo - 1, 3, "e4_f6_s0") == "512" and D.fused_kernel(3 * lo, 3, "e4_f6_s0") == "1024"
    assert D.fused_kernel(3 * lo, 3, "r3_e3_f3_s0") == "1024" and D.fused_kernel(319, None, "f9_s0") == "512"
    assert not D.x_staged(hi - 1, 1) and D.x_staged(hi, 1) and not D.x_staged(2 * hi - 1, 2) and D.x_staged(2 * hi, 2)
    # items: n_obs / kCamItemSpread rounded up to tiles, between kTile and kCamChunk, unless the switch raises the floor
    assert D.camera_items([130, 0, 64], 194)[1].tolist() == [64, 64, 2, 0, 64]
    assert D.camera_items([1100], 1100, 512)[1].tolist() == [512, 512, 76]
    assert D.camera_item_kernel([1100], 1100, "f6_s0", 512) == "mfma" and D.camera_item_kernel([1200], 1200, "f6_s0", 512) == "lane"
    assert D.camera_item_kernel([130, 0, 64], 194, "r4_e4_f2_s0") == "lane"   # rows that are not 2 high: never the matrix-pipe kernel


@pytest.mark.parametrize("name", D.compiled_shapes())
def test_few_cameras_scene(hs, problems, name):
    k = D.constants()
    p = D.few_cameras(problems, name, with_values=False)
    deg, n_tiles = D.camera_degrees(hs, p)
    n_obs = len(p.bs.row_block_size)
    _, lens = D.camera_items(deg, n_obs, D.CAM_CHUNK_MIN)
    sx = hs.debug_staged_x_plan(p.bs, p.num_eliminate_blocks)
    print(f"few cameras {name}: observations {n_obs} (with a camera cell {deg.sum()}) tiles {n_tiles} degrees {deg.tolist()} "
          f"items {len(lens)} (mean {deg.sum() / len(lens):.0f}) staged {len(sx['staged_cam'])} of {sx['n_cameras']}")
    assert 13000 <= n_obs <= 25000 and sx["n_cameras"] == D.FEW_CAMERAS
    assert deg.sum() >= k["kCamItemLaneMinMean"] * int(np.sum(np.maximum(1, -(-deg // D.CAM_CHUNK_MIN)))) == k["kCamItemLaneMinMean"] * len(lens)
    assert D.camera_item_kernel(deg, n_obs, name, D.CAM_CHUNK_MIN) == "lane"
    if D.shape_of(name)[0] == 2:   # by the default rule the items are 64 long: the matrix-pipe kernel
        assert D.camera_item_kernel(deg, n_obs, name) == "mfma"
    assert ((lens != k["kCamChunk"]) & (lens % k["kTile"] != 0) & (lens > k["kTile"])).any(), "no ragged item"
    assert ((lens > 0) & (lens < k["kTile"])).any(), "no item shorter than a wavefront"
    assert (lens == k["kCamChunk"]).sum() >= 20
    assert sorted(sx["staged_cam"].tolist()) == list(range(D.FEW_CAMERAS)), "every camera's x is staged"
    for cap in D.FEW_GRID_CAPS:
        assert n_tiles >= k["kStagedXMinTilesPerWg"] * cap and n_tiles % (8 * cap) != 0, (n_tiles, cap)
        assert D.x_staged(n_tiles, cap) and D.fused_kernel(n_tiles, cap, name) == ("pipelined" if D.pipelined(name) else "1024")
    assert D.fused_kernel(n_tiles, None, name) == "512" and not D.x_staged(n_tiles, None)   # what the scene runs without the cap


@pytest.mark.parametrize("name", D.PIPELINED_SHAPES)
def test_lds_filling_scene(hs, problems, name):
    k = D.constants()
    p = D.lds_filling(problems, name, with_values=False)
    deg, n_tiles = D.camera_degrees(hs, p)
    sx = hs.debug_staged_x_plan(p.bs, p.num_eliminate_blocks)
    n_staged, nf = len(sx["staged_cam"]), D.shape_of(name)[2]
    rows = (sx["slot_word"][sx["slot_word"] >= 0] >> k["kSlotCamBits"])
    mixed = sum(1 for t in (sx["slot_word"].reshape(-1, k["kTile"])) if ((t >= 0) & (t >> k["kSlotCamBits"] > 0)).any() and ((t >= 0) & (t >> k["kSlotCamBits"] == 0)).any())
    print(f"LDS-filling {name}: cameras {sx['n_cameras']} observations {len(p.bs.row_block_size)} tiles {n_tiles} accumulators "
          f"{sx['accumulator_bytes']} B staged rows {n_staged} slots on staged cameras {(rows > 0).sum()} of {rows.size} "
          f"tiles with both kinds of slot {mixed}")
    assert 13000 <= len(p.bs.row_block_size) <= 25000 and sx["n_cameras"] == D.lds_filling_cameras(name)
    assert sx["accumulator_bytes"] + 1024 <= k["kLdsBytesPerCu"], "the accumulators must stay in LDS"
    assert 1 <= n_staged < sx["n_cameras"] and n_staged <= 16
    assert sx["accumulator_bytes"] + 1024 + 8 * nf * (n_staged + 1) > k["kLdsBytesPerCu"], "the staged rows fill what is left"
    assert mixed >= n_tiles // 4, "slots read x from LDS and from memory in the same tile"
    assert n_tiles >= k["kStagedXMinTilesPerWg"] * D.LDS_GRID_CAP and n_tiles % (8 * D.LDS_GRID_CAP) != 0
    assert D.x_staged(n_tiles, D.LDS_GRID_CAP) and D.fused_kernel(n_tiles, D.LDS_GRID_CAP, name) == "pipelined"


def test_boundary_scenes(hs, problems):
    k = D.constants()
    for n_tiles in D.boundary_tiles():
        p = D.boundary(hs, problems, n_tiles)
        deg, got = D.camera_degrees(hs, p)
        print(f"boundary {D.BOUNDARY_SHAPE}: {got} tiles, {len(p.bs.row_block_size)} observations, {D._boundary_points(hs, problems, n_tiles)} points: "
              f"{D.fused_kernel(got, 1, D.BOUNDARY_SHAPE)}, x staged {D.x_staged(got, 1)}")
        assert got == n_tiles
        assert D.fused_kernel(got, D.BOUNDARY_GRID_CAP, D.BOUNDARY_SHAPE) == ("pipelined" if n_tiles >= k["kPipelineMinTilesPerWg"] else "512")
        assert D.x_staged(got, D.BOUNDARY_GRID_CAP) == (n_tiles >= k["kStagedXMinTilesPerWg"])
    assert D.boundary_tiles() == (k["kPipelineMinTilesPerWg"] - 1, k["kPipelineMinTilesPerWg"], k["kStagedXMinTilesPerWg"] - 1, k["kStagedXMinTilesPerWg"])


@pytest.mark.parametrize("name", list(D.LONG_POINT_SHAPES))
def test_long_point_scenes(hs, problems, name):
    k = D.constants()
    p = D.long_points(problems, name, with_values=False)
    deg, n_tiles = D.camera_degrees(hs, p)
    track = np.bincount(p.point_of_row)
    cap = D.long_points_grid_cap(n_tiles)
    print(f"long points {name}: {len(track)} points of {track.min()} .. {track.max()} observations, {n_tiles} tiles, grid cap {cap}: "
          f"{n_tiles / cap:.1f} tiles per workgroup")
    assert (track > k["kTile"]).sum() >= 0.9 * len(track) and track.max() > 4 * k["kTile"], "long points: whole tiles, taken in rounds"
    assert D.pipelined(name) and D.shape_of(name) != (2, 3, 9, 0)
    for c in (cap, D.LONG_POINTS_STAGED_CAP):
        assert D.fused_kernel(n_tiles, c, name) == "pipelined"
    assert not D.x_staged(n_tiles, cap) and D.x_staged(n_tiles, D.LONG_POINTS_STAGED_CAP)
    assert D.fused_kernel(n_tiles, cap + 1, name) == "512", "the cap is the largest that keeps the pipelined kernel"
