"""Motion blur on the MI355X (run with -m gpu): rtHipMotionBlur and rtHipMotionBlurDevice give, bit for bit (a NaN on both sides counts as
equal), the output of the numpy restatement (motion_blur_oracle.py) over the shapes, fields and the parameter grid of
motion_blur_cases.py; the device entry refuses overlaps, bad pointers, a short scratch and foreign streams and launches nothing;
ResidentScene.motion_blur equals the oracle on the scene's own read-back, motion and t for camera moves and geometry updates, does not
move the mark, needs one, makes its storage once and refuses a tile subset; --motion-blur writes what the API returns.  Every test needs
the entry points of this feature, so all of them fail without it."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads its HIP runtime: the order bench.py uses)

import motion_blur_cases as BC
import motion_blur_oracle as BO
import motion_cases as MC
from opencl_render_amd import frontend as F, raytrace as R, scene as S

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the motion blur tests cannot run (and the product has no CPU fallback)")
    MC.use_grid_builder(lambda sc: R.build_scene_grid_device(sc, 0))
    yield
    MC.use_grid_builder(R.build_scene_grid)


def assert_same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, got.dtype)
    bad = np.flatnonzero(~BO.same_bits(got, want).reshape(-1))
    assert bad.size == 0, (f"{label}: differs in {bad.size} of {want.size} values; first {bad[:4]}: got {got.reshape(-1)[bad[:4]]}, "
                           f"want {want.reshape(-1)[bad[:4]]}")


def on_gpu(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")


# ---- synthetic arrays -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, W, H", BC.CASES)
def test_host_and_device_entry_points_equal_the_oracle_bit_for_bit(name, W, H):
    fields = BC.fields(name, W, H)
    dev = [on_gpu(a) for a in fields]
    for params in BC.grid_of(W, H):
        want = BC.reference(name, W, H, params)
        assert_same(R.motion_blur(*fields, **params), want, f"{name} {W}x{H} {params}: numpy")
        got = R.motion_blur(*dev, **params)
        torch.cuda.synchronize()
        assert_same(got.cpu().numpy(), want, f"{name} {W}x{H} {params}: torch")


def test_streams_and_given_outputs():
    name, W, H = "random", 97, 70
    fields, want = BC.fields(name, W, H), BC.reference(name, W, H, BC.GRID[40])
    dev = [on_gpu(a) for a in fields]
    side = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(side):  # a stream of the caller, and twice on it
        got = R.motion_blur(*dev, **BC.GRID[40])
        got = R.motion_blur(*dev, **BC.GRID[40])
    torch.cuda.synchronize()
    assert_same(got.cpu().numpy(), want, "a stream of the caller")
    out = torch.full((H, W, 3), -7.0, device="cuda:0")
    assert R.motion_blur(*dev, **BC.GRID[40], out=out, stream=side.cuda_stream) is out
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), want, "a given output on a given stream")
    host = np.full((H, W, 3), -7.0, F32)
    assert R.motion_blur(*fields, **BC.GRID[40], out=host) is host
    assert_same(host, want, "a given host output")


def test_the_device_entry_refuses_overlaps_bad_pointers_a_short_scratch_and_foreign_streams_and_launches_nothing():
    name, W, H = "random", 65, 34
    fields, want = BC.fields(name, W, H), BC.reference(name, W, H, BC.GRID[40])
    L = R.lib()
    p = R.motion_blur_params(**BC.GRID[40])
    dev = [on_gpu(a) for a in fields]
    need = L.rtHipMotionBlurScratchBytes(W, H)
    out, scratch = torch.full((H, W, 3), -7.0, device="cuda:0"), torch.zeros(need + 64, dtype=torch.uint8, device="cuda:0")
    ptrs = [t.data_ptr() for t in dev] + [out.data_ptr(), scratch.data_ptr()]
    names = ["colour", "motion", "depth", "out", "scratch"]

    def call(stream=None, device=0, scratch_bytes=need, **change):
        args = list(ptrs)
        for k, v in change.items():
            args[names.index(k)] = v
        return L.rtHipMotionBlurDevice(device, W, H, *[C.c_void_p(a) if a else None for a in args], scratch_bytes, C.byref(p), stream)

    host = np.full((H, W, 3), -7.0, F32)
    for k in names:  # a host pointer in any place
        assert call(**{k: host.ctypes.data}) == -1 and "not device memory" in R.last_error() and k in R.last_error(), k
    assert (host == -7.0).all()
    for k in names[:3]:  # the output, or the scratch, on top of an input or inside it
        assert call(out=ptrs[names.index(k)]) == -1 and f"out overlaps {k}" in R.last_error(), k
        assert call(scratch=ptrs[names.index(k)] + 16) == -1 and "scratch overlaps" in R.last_error(), k  # (it may reach a neighbour too)
    assert call(scratch=ptrs[3] + 32) == -1 and "overlaps" in R.last_error()  # the scratch on the output
    assert call(scratch_bytes=need - 1) == -1 and "scratch" in R.last_error() and str(need) in R.last_error()
    assert call(scratch=ptrs[4] + 4) == -1  # not 16-byte aligned
    small = L.rtHipDeviceAlloc(0, need - 16)  # an exact allocation, so that a range past its end is seen
    assert small, R.last_error()
    try:
        assert call(scratch=small) == -1 and "reach past the end" in R.last_error()
    finally:
        L.rtHipDeviceFree(0, C.c_void_p(small))
    if torch.cuda.device_count() > 1:
        other = torch.cuda.Stream(device=1)
        assert call(stream=C.c_void_p(other.cuda_stream)) == -1 and "belongs to device 1" in R.last_error()
        foreign = torch.zeros((H, W), device="cuda:1")  # memory of another device
        assert call(depth=foreign.data_ptr()) == -1 and "depth" in R.last_error()
        torch.cuda.set_device(0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all(), "a refused call wrote its output"
    assert call() == 0
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), want, "after the refusals")


# ---- the scene path -------------------------------------------------------------------------------------------------------------------
def move(rs, sc):
    rs.set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)


def frame_colour(rs):
    """What rtHipSceneMotionBlur gathers, from the host read-back: u16 / 65535."""
    sc = rs.scene
    return np.stack([p.reshape(sc.height, sc.width) for p in rs.readback()], -1).astype(F32) / F32(65535.0)


def blur_step(rs, label):
    """render, motion_blur() under each of SCENE_PARAMS, and the oracle on the scene's own read-back, motion and t.  Returns the share of
    pixels in the gather arm under the first (the defaults)."""
    rs.render()
    before = rs.motion_reference_camera()
    share = None
    for params in BC.SCENE_PARAMS:
        got = rs.motion_blur(**params)
        flow = rs.motion()
        parts = BO.blur(frame_colour(rs), flow["motion"], flow["t"], **params, with_parts=True)
        assert_same(got["rgb"], parts["out"], f"{label} {params}: rgb")
        for ch, g, w in zip("RGB", got["planes"], R.quantise(parts["out"])):
            assert g.dtype == np.uint16 and np.array_equal(g, w), f"{label} {params}: plane {ch}"
        share = float(parts["gathered"].mean()) if share is None else share
    after = rs.motion_reference_camera()
    assert all(np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes() for k in before), f"{label}: the call moved the mark"
    ms = rs.motion_blur_times_ms()
    assert sorted(ms) == ["blur", "gather", "motion"] and all(v >= 0 for v in ms.values()) and ms["blur"] > 0
    return share


@pytest.mark.parametrize("name", list(BC.CAMERA_SCENES))
def test_camera_moves_on_the_scene_path(name):
    sc = MC.base_scene(name, BC.CAMERA_SCENES[name])
    rs = R.ResidentScene(sc, 0)
    try:
        rs.mark_motion()
        shares = {}
        for pose, cur, ref, mark, moves in MC.camera_steps(sc):
            if mark:
                rs.mark_motion()
            move(rs, cur)
            shares[pose] = round(blur_step(rs, f"{name}/{pose}"), 3)
        assert max(shares.values()) >= BC.MIN_GATHER, shares
        assert shares == BC.SCENE_GATHER_SHARES["camera", name]  # the device's flow puts the pixels where the CPU's flow put them
    finally:
        rs.close()


def test_geometry_updates_on_the_scene_path():
    name = BC.GEOMETRY_SCENE
    sc = MC.base_scene(name, MC.GEOMETRY_SCENES[name])
    rs = R.ResidentScene(sc, 0)
    try:
        rs.mark_motion()
        shares = {}
        for change, arrays, cur, ref, mark, moves in MC.geometry_steps(sc):
            if mark:
                rs.mark_motion()
            rs.set_vertices(cur.vertex, cur.tri_index, None)
            shares[change] = round(blur_step(rs, f"{name}/{change}"), 3)
        assert max(shares.values()) >= BC.MIN_GATHER and shares["reindex"] == 0.0, shares  # (reindex: the copy arm, the frame itself)
        assert shares == BC.SCENE_GATHER_SHARES["geometry", name]
    finally:
        rs.close()


def test_the_call_needs_a_mark_keeps_it_and_makes_its_storage_once():
    sc = MC.base_scene("mirror_hall", (24, 16))
    idle = R.ResidentScene(sc, 0)
    rs = R.ResidentScene(sc, 0)
    try:
        idle.render()
        idle.readback()
        rs.render()
        rs.readback()
        bytes0 = rs.bytes()
        assert idle.bytes() == bytes0
        with pytest.raises(RuntimeError, match="no motion reference"):
            rs.motion_blur()
        assert rs.bytes() == bytes0  # a refused call made nothing
        rs.mark_motion()
        move(rs, MC.posed(sc, "pan"))
        rs.render()
        frame = [p.copy() for p in rs.readback()]
        marked = rs.bytes()  # (with the reference and the camera move's storage)
        first = rs.motion_blur()
        grown = rs.bytes()
        n = sc.width * sc.height
        part = lambda b: (b + 255) // 256 * 256  # noqa: E731
        assert grown - marked == (part(n * 8) + part(n * 4) + 2 * part(n * 12) + 3 * part(n * 2)
                                  + part(R.lib().rtHipMotionBlurScratchBytes(sc.width, sc.height)))
        second = rs.motion_blur()
        assert rs.bytes() == grown  # the second call makes nothing more
        assert_same(second["rgb"], first["rgb"], "the second call")
        assert all(np.array_equal(a, b) for a, b in zip(rs.readback(), frame))  # and the frame is what it was
        assert not np.array_equal(first["rgb"], frame_colour(rs))  # (it did blur)
        only = R.lib().rtHipSceneMotionBlur(rs.handle, C.byref(R.motion_blur_params()), None, None, None, None)  # every output left out
        assert only == 0
        assert idle.bytes() == bytes0  # a scene that never calls is the size it was
    finally:
        rs.close()
        idle.close()


def test_scene_refusals_launch_nothing():
    sc = MC.base_scene("axis_near_axis_mixed", MC.CAMERA_SCENES["axis_near_axis_mixed"])  # several tiles
    L = R.lib()
    H, W = sc.height, sc.width
    rgb = np.full((H, W, 3), -7.0, F32)
    planes = [np.full((H, W), 12345, np.uint16) for _ in range(3)]

    def call(rs, params=None):
        return L.rtHipSceneMotionBlur(rs.handle, C.byref(params or R.motion_blur_params()), *[a.ctypes.data_as(C.c_void_p) for a in [rgb] + planes])

    tiles = np.arange(R.tile_count(W, H), dtype=np.uint32)
    for part in (tiles[1:], np.concatenate([tiles, tiles[:1]])):
        rs = R.ResidentScene(sc, 0, part)
        try:
            rs.mark_motion()
            rs.render()
            bytes0 = rs.bytes()
            assert call(rs) == -1 and "every tile of the image" in R.last_error()
            with pytest.raises(RuntimeError, match="every tile of the image"):
                rs.motion_blur()
            assert rs.bytes() == bytes0
        finally:
            rs.close()
    rs = R.ResidentScene(sc, 0)
    try:
        rs.render()
        bytes0 = rs.bytes()
        assert call(rs) == -1 and "no motion reference" in R.last_error()
        rs.mark_motion()
        bytes0 = rs.bytes()
        for bad, word in ((dict(shutter=4.5), "shutter"), (dict(max_blur=0.5), "maxBlur"), (dict(taps=0), "taps"), (dict(taps=65), "taps"),
                          (dict(depth_softness=-1.0), "depthSoftness")):
            assert call(rs, R.motion_blur_params(**bad)) == -1 and word in R.last_error(), bad
            assert rs.bytes() == bytes0
    finally:
        rs.close()
    assert (rgb == -7.0).all() and all((p == 12345).all() for p in planes)


def test_command_line_writes_what_the_api_returns(tmp_path):
    from opencl_render_amd import __main__ as M
    args = ["--scene", "soup", "--width", "64", "--height", "48", "--samples", "1", "--triangles", "20000", "--out", str(tmp_path / "img.bmp")]
    assert M.main(args + ["--orbit", "3", "--motion-blur", str(tmp_path / "mb.pfm"), "--shutter", "1", "--max-blur", "8", "--blur-taps", "9"]) == 0
    assert M.main(args + ["--orbit", "3", "--motion-blur", str(tmp_path / "mb.ppm"), "--temporal", str(tmp_path / "acc.pfm")]) == 0
    sc = S.make_soup(64, 48, 20000, 0.02, samples=1)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    for with_temporal in (False, True):
        rs = R.ResidentScene(sc, 0)
        try:
            blurred = 0
            for i, position in enumerate(R.orbit_positions(np.zeros(3, F32), np.float32([0, 0, 3]), 3)):
                rs.look_at(position, np.float32([0, 0, 3]), (0, 1, 0), np.radians(M.parser().get_default("fov")))
                rs.render()
                if i == 0:
                    rs.mark_motion()
                    want = dict(rgb=frame_colour(rs), planes=[p.reshape(48, 64) for p in rs.readback()])
                else:
                    want = rs.motion_blur() if with_temporal else rs.motion_blur(shutter=1.0, max_blur=8.0, taps=9)
                    blurred += int(not np.array_equal(want["rgb"], frame_colour(rs)))
                if with_temporal:
                    acc = rs.temporal()  # (marks)
                    assert open(tmp_path / f"acc_{i:03d}.pfm", "rb").read() == b"PF\n64 48\n-1.0\n" + acc["colour"][::-1].astype("<f4").tobytes()
                    F.write_ppm(str(tmp_path / "want.ppm"), *want["planes"])
                    assert open(tmp_path / f"mb_{i:03d}.ppm", "rb").read() == open(tmp_path / "want.ppm", "rb").read(), i
                else:
                    rs.mark_motion()
                    assert open(tmp_path / f"mb_{i:03d}.pfm", "rb").read() == b"PF\n64 48\n-1.0\n" + want["rgb"][::-1].astype("<f4").tobytes(), i
            assert blurred == 2  # frame 0 is written as it is, the others are blurred
        finally:
            rs.close()
    with pytest.raises(SystemExit):
        M.parse_args(["--motion-blur", str(tmp_path / "mb.pfm")])
    with pytest.raises(SystemExit):
        M.parse_args(["--orbit", "2", "--motion-blur", str(tmp_path / "mb.png")])
    with pytest.raises(SystemExit):
        M.parse_args(["--orbit", "2", "--shutter", "1"])
    with pytest.raises(SystemExit):
        M.parse_args(["--orbit", "2", "--motion-blur", str(tmp_path / "mb.pfm"), "--blur-taps", "65"])
