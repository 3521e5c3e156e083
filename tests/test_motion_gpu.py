"""Motion vectors on the MI355X (run with -m gpu): rtHipSceneMotion / rtHipSceneMotionDevice give, bit for bit (a NaN on both sides counts
as equal), the four outputs of the numpy restatement (motion_oracle.py, walks by rt_oracle_grid_trace) for camera moves, geometry
updates and both at once against the marked reference (scenes and sequences: motion_cases.py; tests/test_motion.py shows they are not
vacuous); the reference survives two updates; host and device entry points, numpy and torch, foreign streams and output subsets agree;
instances over a tile deal compose and leave other pixels alone; a peer marks for itself; frames, passes, AO and the scene's pointers are
unchanged; refusals launch nothing; a 1M-triangle soup at 1080p agrees with ResidentScene.intersect; --motion writes what the API
returns.  Every test needs the entry points of this feature, so all of them fail without it."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads its HIP runtime: the order bench.py uses)

import motion_cases as MC
import motion_oracle as MO
import scenarios
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu
F32 = np.float32
KEYS = ("motion", "t", "prev_t", "triangle")


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the motion vector tests cannot run (and the product has no CPU fallback)")
    MC.use_grid_builder(lambda sc: R.build_scene_grid_device(sc, 0))
    yield
    MC.use_grid_builder(R.build_scene_grid)


def assert_same(got, want, label, keys=KEYS):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (label, k)
        bad = np.flatnonzero(~MO.same_bits(got[k], want[k]).reshape(-1))
        assert bad.size == 0, (f"{label}: {k} differs in {bad.size} of {want[k].size} values; first {bad[:4]}: got "
                               f"{got[k].reshape(-1)[bad[:4]]}, want {want[k].reshape(-1)[bad[:4]]}")


def move(rs, sc):
    rs.set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)


def sentinels(sc, value=-7.0):
    return dict(motion=np.full((sc.height, sc.width, 2), value, F32), t=np.full((sc.height, sc.width), value, F32),
                prev_t=np.full((sc.height, sc.width), value, F32), triangle=np.full((sc.height, sc.width), 12345, np.uint32))


def device_sentinels(sc, value=-7.0):
    dev = torch.device("cuda", 0)
    return {k: torch.as_tensor(v.view(np.int32) if k == "triangle" else v, device=dev) for k, v in sentinels(sc, value).items()}


def to_numpy(out):
    return {k: (v.cpu().numpy().view(np.uint32) if k == "triangle" else v.cpu().numpy()) for k, v in out.items()}


@pytest.mark.parametrize("name", list(MC.CAMERA_SCENES))
def test_camera_moves(name):
    sc = MC.base_scene(name, MC.CAMERA_SCENES[name])
    rs = R.ResidentScene(sc, 0)
    try:
        rs.mark_motion()
        assert_same(rs.motion(), MO.motion(sc, sc), f"{name}: marked and measured at home")
        for pose, cur, ref, mark, moves in MC.camera_steps(sc):
            if mark:
                rs.mark_motion()
            cam = rs.motion_reference_camera()
            for k in ("eye", "eye_to_top_left", "left_to_right", "top_to_bottom"):
                assert cam[k][:3].tobytes() == np.asarray(getattr(ref, k), F32)[:3].tobytes(), (pose, k)
            move(rs, cur)
            assert_same(rs.motion(), MO.motion(cur, ref), f"{name}/{pose}")
    finally:
        rs.close()


@pytest.mark.parametrize("name", list(MC.GEOMETRY_SCENES))
def test_geometry_updates(name):
    sc = MC.base_scene(name, MC.GEOMETRY_SCENES[name])
    rs = R.ResidentScene(sc, 0)
    try:
        rs.mark_motion()
        since_mark = 0
        for change, arrays, cur, ref, mark, moves in MC.geometry_steps(sc):
            if mark:
                rs.mark_motion()
                since_mark = 0
            rs.set_vertices(cur.vertex, cur.tri_index, None)
            since_mark += 1
            got = rs.motion()
            assert_same(got, MO.motion(cur, ref), f"{name}/{change} ({since_mark} updates since the mark)")
            if change == "reindex":
                assert_same(got, MO.motion(cur, cur), f"{name}/{change}: the same-state motion")
            if change == "twist":
                assert since_mark == 2  # the reference is still the marked shape, not the update's spare set
    finally:
        rs.close()


def test_camera_and_geometry_changed_between_mark_and_call():
    sc, arrays, cur, ref = MC.mixed_case()
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_pipeline(R.PIPELINE_MEGAKERNEL)  # (the pass does not depend on the pipeline)
        rs.mark_motion()
        rs.set_vertices(cur.vertex, cur.tri_index, None)
        move(rs, cur)
        assert_same(rs.motion(), MO.motion(cur, ref), "twist + pan")
    finally:
        rs.close()


@pytest.fixture(scope="module")
def pair():
    """(base, current, oracle outputs) of a multi-tile scene moved after its mark."""
    sc = MC.base_scene("axis_near_axis_mixed", MC.CAMERA_SCENES["axis_near_axis_mixed"])
    cur = MC.posed(sc, "pan")
    return sc, cur, MO.motion(cur, sc)


def test_host_device_numpy_torch_streams_and_subsets_agree(pair):
    sc, cur, want = pair
    rs = R.ResidentScene(sc, 0)
    dev = torch.device("cuda", 0)
    try:
        rs.mark_motion()
        move(rs, cur)
        assert_same(rs.motion(), want, "host entry")
        out = device_sentinels(sc)
        assert rs.motion(out=out) is out
        torch.cuda.synchronize()
        assert_same(to_numpy(out), want, "device entry (torch, current stream)")
        side = torch.cuda.Stream(dev)  # a foreign stream, and twice on it
        out2 = device_sentinels(sc)
        with torch.cuda.stream(side):
            rs.motion(out=out2)
            rs.motion(out=out2)
        torch.cuda.synchronize()
        assert_same(to_numpy(out2), want, "device entry (foreign stream)")
        for keys in (("motion",), ("t", "triangle"), ("prev_t",), ("motion", "prev_t", "triangle")):  # any subset may be NULL
            host = {k: v for k, v in sentinels(sc).items() if k in keys}
            got = rs.motion(out=host)
            assert sorted(got) == sorted(keys)
            assert_same(got, want, f"host subset {keys}", keys)
            devs = {k: v for k, v in device_sentinels(sc).items() if k in keys}
            rs.motion(out=devs)
            torch.cuda.synchronize()
            assert_same(to_numpy(devs), want, f"device subset {keys}", keys)
        with pytest.raises(ValueError):
            rs.motion(out={})
        with pytest.raises(ValueError):
            rs.motion(out=dict(t=np.zeros((sc.height, sc.width), np.float64)))
        with pytest.raises(ValueError):
            rs.motion(out=dict(motion=torch.zeros((sc.height, sc.width), device=dev)))
    finally:
        rs.close()


def test_instances_over_a_tile_deal_compose_and_a_peer_marks_for_itself(pair):
    sc, cur, want = pair
    parts, host, devout = [], sentinels(sc), device_sentinels(sc)
    try:
        for rank in range(2):
            tiles = R.tiles_of_rank(sc.width, sc.height, rank, 2)
            parts.append(R.ResidentScene(sc, 0, tiles, like=parts[0] if parts else None))
        parts[0].mark_motion()
        with pytest.raises(RuntimeError):  # the peer has no reference of its own yet
            parts[1].motion()
        assert "no motion reference" in R.last_error()
        parts[1].mark_motion()
        for rank, rs in enumerate(parts):
            move(rs, cur)
            rs.motion(out=host)
            rs.motion(out=devout)
            torch.cuda.synchronize()
            if rank == 0:  # only this instance's tiles are written
                mine = np.zeros((sc.height, sc.width), bool)
                for t in rs.tiles:
                    ty, tx = divmod(int(t), (sc.width + R.TILE - 1) // R.TILE)
                    mine[ty * R.TILE:(ty + 1) * R.TILE, tx * R.TILE:(tx + 1) * R.TILE] = True
                assert mine.any() and not mine.all()
                first, keep = to_numpy(devout), sentinels(sc)
                for k in KEYS:
                    assert MO.same_bits(host[k][~mine], keep[k][~mine]).all() and MO.same_bits(first[k][~mine], keep[k][~mine]).all(), k
                    assert MO.same_bits(host[k][mine], want[k][mine]).all(), k
    finally:
        for p in parts:
            p.close()
    assert_same(host, want, "two instances composed (host)")
    assert_same(to_numpy(devout), want, "two instances composed (device)")


def test_host_and_device_entries_agree_on_shuffled_partial_tiles():
    """Slot order that is not image order, one slot mostly outside the image: the host entry point's arrays are the device entry
    point's, bit for bit, other tiles' pixels left alone by both."""
    sc, tiles = scenarios.shuffled_tiles(), scenarios.SHUFFLED_TILES
    host, devout = sentinels(sc), device_sentinels(sc)
    rs = R.ResidentScene(sc, 0, tiles)
    try:
        rs.mark_motion()
        cam = rs.camera()
        cam["eye"] = cam["eye"] + np.asarray(cam["left_to_right"], F32) * F32(3.0)  # a small pan after the mark
        rs.set_camera(**cam)
        rs.motion(out=host)
        rs.motion(out=devout)
        torch.cuda.synchronize()
    finally:
        rs.close()
    mine, keep = scenarios.tiles_mask(sc, tiles), sentinels(sc)
    assert_same(host, to_numpy(devout), "tiles 3, 0")
    for k in KEYS:
        assert MO.same_bits(host[k][~mine], keep[k][~mine]).all(), k
    seen = host["triangle"] != 0xFFFFFFFF
    assert seen[128:, 128:].any() and seen[:128, :128].any()  # both tiles show something


def test_nothing_else_changes():
    sc = MC.base_scene("mirror_hall", (24, 16))
    cur = MC.posed(sc, "pan")
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(alpha=True, depth=True, triangle=True, normal=True, albedo=True)
        move(rs, cur)
        rs.render()
        planes, passes = rs.readback(), rs.readback_passes()
        ao = rs.ambient_occlusion(rays=4, seed=3)
        pointers, bytes0 = rs.pointers(), rs.bytes()
        rs.mark_motion()
        bytes1 = rs.bytes()
        assert rs.pointers() == pointers
        assert 0 < bytes1 - bytes0 <= max(64 * sc.triangle_count, 16)  # the reference: at most 64 B per triangle
        rs.motion()
        bytes2 = rs.bytes()
        assert bytes2 - bytes1 == 20 * len(rs.tiles) * R.TILE * R.TILE  # the host entry point's staging, as the header documents
        rs.mark_motion()
        rs.motion()
        rs.motion(out=device_sentinels(sc))
        torch.cuda.synchronize()
        assert rs.bytes() == bytes2 and rs.pointers() == pointers
        rs.render()
        assert all(np.array_equal(a, b) for a, b in zip(planes, rs.readback()))
        again = rs.readback_passes()
        for k in passes:
            assert np.array_equal(np.asarray(passes[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8)), k
        assert np.array_equal(ao.view(np.uint32), rs.ambient_occlusion(rays=4, seed=3).view(np.uint32))
    finally:
        rs.close()


def test_refusals_launch_nothing(pair):
    sc, cur, want = pair
    L = R.lib()
    rs = R.ResidentScene(sc, 0)
    try:
        out, host = device_sentinels(sc), sentinels(sc)
        dp = [C.c_void_p(out[k].data_ptr()) for k in KEYS]
        hp = [host[k].ctypes.data_as(C.c_void_p) for k in KEYS]
        cam = R.Camera()
        # before a mark
        assert L.rtHipSceneMotionReferenceCamera(rs.handle, C.byref(cam)) == -1
        assert L.rtHipSceneMotionDevice(rs.handle, *dp, None) == -1 and "no motion reference" in R.last_error()
        assert L.rtHipSceneMotion(rs.handle, *hp) == -1 and "no motion reference" in R.last_error()
        bytes0 = rs.bytes()
        rs.mark_motion()
        # every output NULL, a NULL scene, a host pointer for the device entry
        assert L.rtHipSceneMotionDevice(rs.handle, None, None, None, None, None) == -1 and "null" in R.last_error()
        assert L.rtHipSceneMotion(rs.handle, None, None, None, None) == -1 and "null" in R.last_error()
        assert L.rtHipSceneMotionDevice(None, *dp, None) == -1
        for i in range(4):
            mixed = list(dp)
            mixed[i] = hp[i]
            assert L.rtHipSceneMotionDevice(rs.handle, *mixed, None) == -1
            assert "not device memory" in R.last_error()
        torch.cuda.synchronize()
        got, keep = to_numpy(out), sentinels(sc)
        for k in KEYS:
            assert MO.same_bits(got[k], keep[k]).all() and MO.same_bits(host[k], keep[k]).all(), k
        assert rs.bytes() - bytes0 <= max(64 * sc.triangle_count, 16)  # (no staging was made by a refused call)
    finally:
        rs.close()


def test_million_triangle_soup_at_1080p_against_intersect():
    sc = S.make_soup(1920, 1080, 1_000_000, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    cur = MC.posed(sc, "pan")
    rs = R.ResidentScene(sc, 0)
    try:
        rs.mark_motion()
        move(rs, cur)
        got = rs.motion()

        def walk(rays):
            return rs.intersect(rays["o"], rays["d"], rays["tmin"], rays["tmax"], rays["excluded"])

        want = MO.motion(cur, sc, walk=walk)
    finally:
        rs.close()
    hit, far, _ = MC.shares(want)
    assert hit > 0.2 and far > 0.1  # the image is not just misses, and the pan moves it
    assert_same(got, want, "soup_1m 1080p")


def test_command_line_writes_what_the_api_returns(tmp_path):
    from opencl_render_amd import __main__ as M
    args = ["--scene", "soup", "--width", "64", "--height", "48", "--samples", "1", "--triangles", "20000", "--out", str(tmp_path / "img.bmp")]
    assert M.main(args + ["--orbit", "3", "--motion", str(tmp_path / "mv")]) == 0
    sc = S.make_soup(64, 48, 20000, 0.02, samples=1)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc, 0)
    try:
        moved = 0
        for i, position in enumerate(R.orbit_positions(np.zeros(3, F32), np.float32([0, 0, 3]), 3)):
            rs.look_at(position, np.float32([0, 0, 3]), (0, 1, 0), np.radians(M.parser().get_default("fov")))
            if i == 0:
                rs.mark_motion()
            want = rs.motion()
            rs.mark_motion()
            with np.load(tmp_path / f"mv_{i:03d}.npz") as z:
                assert sorted(z.files) == sorted(KEYS)
                assert_same({k: z[k] for k in KEYS}, want, f"--motion frame {i}")
            hit, far, _ = MC.shares(want)
            assert hit > 0
            moved += far > 0.1
        assert moved == 2  # frame 0 is measured against itself, the others against the view before
    finally:
        rs.close()
    with pytest.raises(SystemExit):
        M.parse_args(["--motion", str(tmp_path / "mv")])
