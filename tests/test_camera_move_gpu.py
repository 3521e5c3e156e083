"""rtHipSceneSetCamera on the device: a resident scene moved to a new camera is the scene a fresh upload would have made.

The oracle is never the code under test: for a pose, a copy of the Scene with the camera fields replaced, the lists of
oracle_lib.oracle_camera_list (the serial restatement of the reference's builder) and the planes of oracle_lib.oracle_render.  Poses
and list helpers: tests/camera_cases.py.  Every test here needs the entry points of this feature, so all of them fail without it."""
import copy
import os

import numpy as np
import pytest

import builder_cases as BC
import camera_cases as CC
import oracle_lib as O
import scenarios
from opencl_render_amd import raytrace as R

pytestmark = pytest.mark.gpu

THREADS = min(os.cpu_count() or 1, 16)


def base_scene(name):
    sc = getattr(scenarios, name)()
    R.build_scene_grid(sc)  # (the grid does not depend on the camera)
    return CC.posed(sc, "home")


def oracle_planes(sc):
    return [p.reshape(-1) for p in O.oracle_render(sc, threads=THREADS)]


def frame(rs):
    rs.render()
    return rs.readback()


def assert_planes(got, want, label):
    for ch, g, w in zip("RGB", got, want):
        bad = np.nonzero(np.asarray(g).reshape(-1) != np.asarray(w).reshape(-1))[0]
        assert bad.size == 0, f"{label}: plane {ch} differs in {bad.size} pixels, first {bad[:5]}"


def move(rs, sc):
    rs.set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)


@pytest.fixture(scope="module")
def posed_scenes():
    """name -> (base scene, {pose: Scene with the oracle's lists, its oracle planes})"""
    out = {}
    for name in CC.SCENES:
        sc = base_scene(name)
        poses = {}
        for pose in CC.POSES:
            p = CC.posed(sc, pose)
            poses[pose] = (p, oracle_planes(p))
        out[name] = (sc, poses)
    return out


@pytest.mark.parametrize("pipeline", [R.PIPELINE_WAVEFRONT, R.PIPELINE_MEGAKERNEL] if hasattr(R, "PIPELINE_WAVEFRONT") else [1, 0])
@pytest.mark.parametrize("name", CC.SCENES)
def test_frames_and_lists_follow_the_camera(posed_scenes, name, pipeline):
    """1 + 2: planes of every pose equal the oracle's as integers, every pixel's list equals the oracle list's slice, the last pose
    (the original one) gives the scene's first frame again; both pipelines."""
    sc, poses = posed_scenes[name]
    shares = [CC.share_non_empty(poses[p][0]) for p in CC.POSES]
    assert sum(s >= CC.MIN_SHARE for s in shares) >= 3, f"{name}: non-empty shares {shares}: the poses would pass on blank frames"
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_pipeline(pipeline)
        first = frame(rs)
        assert_planes(first, poses["home"][1], f"{name}: first frame")
        for pose in CC.POSES:
            want, planes = poses[pose]
            move(rs, want)
            cam = rs.camera()
            assert cam["eye"].tobytes() == want.eye.tobytes() and cam["left_to_right"].tobytes() == want.left_to_right.tobytes()
            assert cam["pixel_size_inv"] == want.pixel_size_inv
            CC.assert_lists_equal(rs, want, f"{name}/{pose}")
            assert_planes(frame(rs), planes, f"{name}/{pose}, pipeline {pipeline}")
        assert_planes(frame(rs), first, f"{name}: back at the original pose")
    finally:
        rs.close()


def test_builder_families():
    """3: every family of tests/builder_cases.py, created with a shifted camera and moved to the family's own; over the families both the
    per-thread and the per-workgroup rasteriser ran and the logged entries are the oracle's per-pixel lengths summed."""
    threads = groups = 0
    for name in BC.NAMES:
        sc = BC.make(name)
        R.build_scene_grid(sc)
        home, shifted = CC.posed(sc, "home"), CC.posed(sc, "shifted")
        rs = R.ResidentScene(shifted, 0)
        try:
            assert rs.camera_log() == dict(thread=0, group=0, entries=0)
            move(rs, home)
            entries = CC.assert_lists_equal(rs, home, f"family {name}")
            log = rs.camera_log()
            assert log["entries"] == entries, f"family {name}: logged {log['entries']} entries, the oracle's lists sum to {entries}"
            assert log["thread"] + log["group"] == sc.triangle_count
            threads += log["thread"]; groups += log["group"]
            move(rs, shifted)
            CC.assert_lists_equal(rs, shifted, f"family {name}, back to the shifted camera")
        finally:
            rs.close()
    assert threads > 0 and groups > 0, f"per-thread {threads}, per-workgroup {groups}: one of the two rasterisers never ran"
    assert len(R.build_log()) >= 1  # (the move leaves the public builders' log alone; its own log is camera_log())


def test_tile_subsets(posed_scenes):
    """4: two instances over a round-robin deal, both moved: the composed planes are the oracle's, each keeps its tiles."""
    sc, poses = posed_scenes["odd_size_multi_tile"]
    want, planes = poses["orbit90"]
    assert CC.share_non_empty(want) >= CC.MIN_SHARE
    a = R.ResidentScene(sc, 0, tiles=R.tiles_of_rank(sc.width, sc.height, 0, 2))
    b = R.ResidentScene(sc, 0, tiles=R.tiles_of_rank(sc.width, sc.height, 1, 2), like=a)
    try:
        counts = [a.scene_header()["tile_count"], b.scene_header()["tile_count"]]
        assert counts == [len(a.tiles), len(b.tiles)] and sum(counts) == R.tile_count(sc.width, sc.height)
        got = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
        total = 0
        for rs in (a, b):
            move(rs, want)
            total += CC.assert_lists_equal(rs, want, f"tiles {rs.tiles.tolist()}")  # only its tiles: the arrays have tile_count * 128 * 128 ranges
            rs.render()
            rs.readback(got)
        assert [a.scene_header()["tile_count"], b.scene_header()["tile_count"]] == counts
        assert total == int((want.cam_end.astype(np.int64) - want.cam_start).sum()) == a.camera_log()["entries"] + b.camera_log()["entries"]
        assert_planes(got, planes, "two instances composed")
    finally:
        b.close(); a.close()


def test_nothing_else_moves(posed_scenes):
    """5: the other parts stay where they are, and a second move to a view of no more entries allocates nothing."""
    sc, poses = posed_scenes["odd_size_multi_tile"]
    rs = R.ResidentScene(sc, 0)
    try:
        before = rs.pointers()
        assert all(before[:5]), before
        big, small = poses["inside"][0], poses["pan"][0]
        move(rs, big)
        n_big = rs.camera_log()["entries"]
        bytes_first = rs.bytes()
        assert rs.pointers() == before
        move(rs, small)
        assert rs.camera_log()["entries"] <= n_big
        assert rs.bytes() == bytes_first
        move(rs, big)
        assert rs.bytes() == bytes_first and rs.pointers() == before
        assert_planes(frame(rs), poses["inside"][1], "after three moves")
    finally:
        rs.close()


def test_passes_denoise_and_ao_follow_the_camera(posed_scenes):
    """6: with all five passes on, a moved scene's passes, denoised image and AO image are those of a fresh scene at the pose (the
    project's numpy oracles pin the fresh scene elsewhere); ray queries and the bake do not read the camera."""
    sc, poses = posed_scenes["mixed_materials_textured"]
    want = poses["orbit90"][0]
    on = dict(alpha=True, depth=True, triangle=True, normal=True, albedo=True)
    rng = np.random.default_rng(5)
    origins = np.tile(np.array([0.0, 0.0, 0.0], np.float32), (64, 1))
    directions = np.concatenate([rng.uniform(-0.4, 0.4, (64, 2)), np.ones((64, 1))], 1).astype(np.float32)
    moved, fresh = R.ResidentScene(sc, 0), R.ResidentScene(want, 0)
    try:
        for rs in (moved, fresh):
            rs.set_passes(**on)
        frame(moved)
        hits0 = moved.intersect(origins, directions)
        bake0 = moved.bake_ambient_occlusion(32, 32, rays=4, seed=2)
        move(moved, want)
        results = []
        for rs in (moved, fresh):
            planes = frame(rs)
            results.append((planes, rs.readback_passes(), rs.denoise(), rs.ambient_occlusion(rays=4, pixel_samples=2, seed=3)))
        (pm, passes_m, den_m, ao_m), (pf, passes_f, den_f, ao_f) = results
        assert_planes(pm, pf, "beauty")
        assert_planes(pm, poses["orbit90"][1], "beauty against the oracle")
        assert CC.share_non_empty(want) >= CC.MIN_SHARE and passes_f["alpha"].any() and np.isfinite(passes_f["depth"]).any()  # not a blank view
        for k in ("alpha", "depth", "triangle", "material", "normal", "albedo"):
            assert passes_m[k].tobytes() == passes_f[k].tobytes(), f"pass {k} differs"
        assert den_m["colour"].tobytes() == den_f["colour"].tobytes()
        assert_planes(den_m["planes"], den_f["planes"], "denoised planes")
        assert ao_m.tobytes() == ao_f.tobytes() and ao_f.any()
        hits1 = moved.intersect(origins, directions)
        for k in hits0:
            assert np.asarray(hits0[k]).tobytes() == np.asarray(hits1[k]).tobytes(), f"ray query field {k} changed with the camera"
        bake1 = moved.bake_ambient_occlusion(32, 32, rays=4, seed=2)
        assert bake0["ao"].tobytes() == bake1["ao"].tobytes() and bake0["triangle"].tobytes() == bake1["triangle"].tobytes()
    finally:
        moved.close(); fresh.close()


def test_planned_frames_after_a_move(posed_scenes):
    """7: the old view's launch plan is dropped: the watched frame after a move logs the rounds of a fresh scene at the pose, and the
    planned frames after it are complete.  (A redo reported by finish() is legal.)"""
    sc, poses = posed_scenes["mirror_hall"]
    want, planes = poses["inside"]
    moved, fresh = R.ResidentScene(sc, 0), R.ResidentScene(want, 0)
    try:
        for _ in range(2):  # a watched frame and a planned one at the old pose
            frame(moved)
        move(moved, want)
        assert_planes(frame(moved), planes, "frame 1 after the move (watched)")
        assert_planes(frame(fresh), planes, "fresh scene")
        assert moved.round_rays(16) == fresh.round_rays(16)
        for i in (2, 3):
            moved.render()
            moved.sync()
            moved.finish()
            assert_planes(moved.readback(), planes, f"frame {i} after the move (planned)")
    finally:
        moved.close(); fresh.close()


def test_refusal_is_transactional(posed_scenes):
    """8: a move above the list limit returns -3 and leaves the scene as it was; with the limit restored the same move succeeds."""
    sc, poses = posed_scenes["odd_size_multi_tile"]
    old, old_planes = poses["pan"]
    new, new_planes = poses["inside"]
    total = int((new.cam_end.astype(np.int64) - new.cam_start).sum())
    rs = R.ResidentScene(sc, 0)
    try:
        move(rs, old)
        ptrs = rs.pointers()
        R.tune("build_list_limit", total - 1)
        try:
            rc = rs.try_set_camera(new.eye, new.eye_to_top_left, new.left_to_right, new.top_to_bottom, new.pixel_size_inv)
            assert rc == -3 and R.last_error()
            cam = rs.camera()
            assert cam["eye"].tobytes() == old.eye.tobytes() and cam["eye_to_top_left"].tobytes() == old.eye_to_top_left.tobytes()
            CC.assert_lists_equal(rs, old, "after the refused move")
            assert_planes(frame(rs), old_planes, "after the refused move")
            assert rs.pointers() == ptrs
            R.tune("build_list_limit", total)  # exactly the view's entries: legal
            assert rs.try_set_camera(new.eye, new.eye_to_top_left, new.left_to_right, new.top_to_bottom, new.pixel_size_inv) == 0
        finally:
            R.tune("build_list_limit", 0xFFFFFFFF)
        CC.assert_lists_equal(rs, new, "after the limit was restored")
        assert_planes(frame(rs), new_planes, "after the limit was restored")
        assert rs.pointers() == ptrs
    finally:
        rs.close()


ODD = {  # legal and defined: the answer is the host builder's for the same values (it shares the membership header)
    "nan_eye": dict(eye=(np.nan, 0.0, 0.0)),
    "zero_pixel_size_inv": dict(pixel_size_inv=0.0),
    "infinite_left_to_right": dict(left_to_right=(np.inf, 0.0, 0.0)),
}


@pytest.mark.parametrize("case", list(ODD))
def test_odd_cameras(posed_scenes, case):
    """9: NaN eye, pixelSizeInv 0, infinite leftToRight: the move succeeds, the lists are raytrace.build_camera_list's for the same
    values (checked on the CPU: the host builder takes all three), and a frame afterwards completes."""
    sc, _ = posed_scenes["lambert_distant"]
    want = copy.copy(sc)
    for k, v in ODD[case].items():
        if k == "pixel_size_inv":
            want.pixel_size_inv = float(v)
        else:
            row = np.zeros(4, np.float32)
            row[:3] = v
            setattr(want, k, row)
    R.build_camera_list(want)
    rs = R.ResidentScene(sc, 0)
    try:
        assert rs.try_set_camera(want.eye, want.eye_to_top_left, want.left_to_right, want.top_to_bottom, want.pixel_size_inv) == 0, R.last_error()
        CC.assert_lists_equal(rs, want, case)
        rs.render()
        rs.sync()
        rs.finish()
        assert len(rs.readback()) == 3
    finally:
        rs.close()
