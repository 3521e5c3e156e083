"""Depth of field on the MI355X (run with -m gpu): rtHipDepthOfField and rtHipDepthOfFieldDevice give, bit for bit (a NaN on both sides
counts as equal), the output of the numpy restatement (dof_oracle.py) over the shapes, fields and the parameter grid of dof_cases.py;
the device entry writes nothing outside W x H, takes a scratch full of garbage, and refuses overlaps, bad pointers, a short scratch and
foreign streams and launches nothing; ResidentScene.depth_of_field equals the oracle on the scene's own read-back and depth pass, also
after set_camera and set_vertices, and on a scene of four scene tiles (the gather's slot > 0 and tilesX > 1), needs the depth pass
and every tile, makes its storage once and leaves the scene as a twin that never calls it; --dof writes what the API returns.  Every
test needs the entry points of this feature, so all of them fail without it."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads its HIP runtime: the order bench.py uses)

import dof_cases as DC
import dof_oracle as DO
import motion_cases as MC
from opencl_render_amd import frontend as F, raytrace as R, scene as S

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the depth of field tests cannot run (and the product has no CPU fallback)")
    MC.use_grid_builder(lambda sc: R.build_scene_grid_device(sc, 0))
    yield
    MC.use_grid_builder(R.build_scene_grid)


def assert_same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, got.dtype)
    bad = np.flatnonzero(~DO.same_bits(got, want).reshape(-1))
    assert bad.size == 0, (f"{label}: differs in {bad.size} of {want.size} values; first {bad[:4]}: got {got.reshape(-1)[bad[:4]]}, "
                           f"want {want.reshape(-1)[bad[:4]]}")


def on_gpu(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")


# ---- synthetic arrays -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, W, H", DC.CASES)
def test_host_and_device_entry_points_equal_the_oracle_bit_for_bit(name, W, H):
    fields = DC.fields(name, W, H)
    dev = [on_gpu(a) for a in fields]
    for params in DC.grid_of(W, H):
        want = DC.reference(name, W, H, params)
        assert_same(R.depth_of_field(*fields, **params), want, f"{name} {W}x{H} {params}: numpy")
        got = R.depth_of_field(*dev, **params)
        torch.cuda.synchronize()
        assert_same(got.cpu().numpy(), want, f"{name} {W}x{H} {params}: torch")


def test_streams_and_given_outputs():
    name, W, H = "layers", 64, 40
    params = DC.ORDINARY[6]
    fields, want = DC.fields(name, W, H), DC.reference(name, W, H, params)
    dev = [on_gpu(a) for a in fields]
    side = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(side):  # a stream of the caller, and twice on it
        got = R.depth_of_field(*dev, **params)
        got = R.depth_of_field(*dev, **params)
    torch.cuda.synchronize()
    assert_same(got.cpu().numpy(), want, "a stream of the caller")
    out = torch.full((H, W, 3), -7.0, device="cuda:0")
    assert R.depth_of_field(*dev, **params, out=out, stream=side.cuda_stream) is out
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), want, "a given output on a given stream")
    host = np.full((H, W, 3), -7.0, F32)
    assert R.depth_of_field(*fields, **params, out=host) is host
    assert_same(host, want, "a given host output")


@pytest.mark.parametrize("name, W, H", [("split",) + DC.WIDE, ("layers", 31, 9), ("ramp", 1, 1)])
def test_out_is_untouched_outside_the_image_and_the_scratch_may_hold_garbage(name, W, H):
    L = R.lib()
    fields = DC.fields(name, W, H)
    dev = [on_gpu(a) for a in fields]
    need = L.rtHipDepthOfFieldScratchBytes(W, H)
    pad = 64  # floats before and after the image
    for params in (DC.DEFAULT_LIKE, DC.ORDINARY[5]):
        for garbage in (0xFF, 0x7F, 0x00):  # NaNs of both signs' patterns, huge values, zeros
            out = torch.full((pad + H * W * 3 + pad,), -7.0, device="cuda:0")
            scratch = torch.full((need + 32,), garbage, dtype=torch.uint8, device="cuda:0")
            p = R.dof_params(**params)
            rc = L.rtHipDepthOfFieldDevice(0, W, H, C.c_void_p(dev[0].data_ptr()), C.c_void_p(dev[1].data_ptr()),
                                           C.c_void_p(out.data_ptr() + 4 * pad), C.c_void_p(scratch.data_ptr()), need, C.byref(p), None)
            assert rc == 0, R.last_error()
            torch.cuda.synchronize()
            flat = out.cpu().numpy()
            assert (flat[:pad] == -7.0).all() and (flat[-pad:] == -7.0).all(), "the filter wrote outside W x H"
            assert_same(flat[pad:-pad].reshape(H, W, 3), DC.reference(name, W, H, params), f"{name} {params} garbage {garbage:#x}")
            assert (scratch[need:].cpu().numpy() == garbage).all(), "the filter wrote past its scratch"


def test_the_device_entry_refuses_overlaps_bad_pointers_a_short_scratch_and_foreign_streams_and_launches_nothing():
    name, W, H = "layers", 64, 40
    params = DC.ORDINARY[6]
    fields, want = DC.fields(name, W, H), DC.reference(name, W, H, params)
    L = R.lib()
    p = R.dof_params(**params)
    dev = [on_gpu(a) for a in fields]
    need = L.rtHipDepthOfFieldScratchBytes(W, H)
    out, scratch = torch.full((H, W, 3), -7.0, device="cuda:0"), torch.zeros(need + 64, dtype=torch.uint8, device="cuda:0")
    ptrs = [t.data_ptr() for t in dev] + [out.data_ptr(), scratch.data_ptr()]
    names = ["colour", "depth", "out", "scratch"]

    def call(stream=None, device=0, scratch_bytes=need, **change):
        args = list(ptrs)
        for k, v in change.items():
            args[names.index(k)] = v
        return L.rtHipDepthOfFieldDevice(device, W, H, *[C.c_void_p(a) if a else None for a in args], scratch_bytes, C.byref(p), stream)

    host = np.full((H, W, 3), -7.0, F32)
    for k in names:  # a host pointer in any place
        assert call(**{k: host.ctypes.data}) == -1 and "not device memory" in R.last_error() and k in R.last_error(), k
    assert (host == -7.0).all()
    for k in names[:2]:  # the output, or the scratch, on top of an input or inside it
        assert call(out=ptrs[names.index(k)]) == -1 and f"out overlaps {k}" in R.last_error(), k
        assert call(scratch=ptrs[names.index(k)] + 16) == -1 and "scratch overlaps" in R.last_error(), k  # (it may reach a neighbour too)
    assert call(scratch=ptrs[2] + 32) == -1 and "overlaps" in R.last_error()  # the scratch on the output
    assert call(scratch_bytes=need - 1) == -1 and "scratch" in R.last_error() and str(need) in R.last_error()
    assert call(scratch=ptrs[3] + 4) == -1  # not 16-byte aligned
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
SCENE, SIZE = "mirror_hall", (24, 16)  # the smallest scene the other scene tests use
SCENE_PARAMS = DC.SCENE_PARAMS


def move(rs, sc):
    rs.set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)


def frame_colour(rs):
    """What rtHipSceneDepthOfField gathers, from the host read-back: u16 / 65535."""
    sc = rs.scene
    return np.stack([p.reshape(sc.height, sc.width) for p in rs.readback()], -1).astype(F32) / F32(65535.0)


def focus_of(depth):
    """A distance in focus that leaves pixels on both sides of it: the median of the depths that hit."""
    hit = depth[np.isfinite(depth) & (depth > 0)]
    assert hit.size, "the frame hit nothing"
    return float(np.median(hit))


def dof_step(rs, label):
    """render, depth_of_field() under each of SCENE_PARAMS, and the oracle on the scene's own read-back and depth pass.  Returns the share
    of pixels in the gather arm under the first."""
    rs.render()
    depth = rs.readback_passes()["depth"]
    colour = frame_colour(rs)
    share = None
    for params in SCENE_PARAMS:
        got = rs.depth_of_field(focus=focus_of(depth), **params)
        parts = DO.blur(colour, depth, **got["params"], with_parts=True)
        assert_same(got["rgb"], parts["out"], f"{label} {params}: rgb")
        for ch, g, w in zip("RGB", got["planes"], R.quantise(parts["out"])):
            assert g.dtype == np.uint16 and np.array_equal(g, w), f"{label} {params}: plane {ch}"
        share = float(parts["gathered"].mean()) if share is None else share
        assert not DO.same_bits(parts["out"], colour).all(), f"{label} {params}: nothing was blurred"
    ms = rs.depth_of_field_times_ms()
    assert sorted(ms) == ["blur", "gather", "output"] and all(v > 0 for v in ms.values()), ms
    return share


def test_the_scene_path_equals_the_oracle_also_after_set_camera_and_set_vertices():
    sc = MC.base_scene(SCENE, SIZE)
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(depth=True)
        assert rs.depth_of_field_times_ms() == dict(gather=0.0, blur=0.0, output=0.0)  # zero before the first call
        shares = [dof_step(rs, f"{SCENE}/home")]
        move(rs, MC.posed(sc, "pan"))
        shares.append(dof_step(rs, f"{SCENE}/pan"))
        _, twisted = MC.shaped(sc, "twist")
        rs.set_vertices(twisted.vertex, twisted.tri_index, None)
        shares.append(dof_step(rs, f"{SCENE}/pan/twist"))
        assert min(shares) >= DC.MIN_GATHER, shares
        # the lens and the pixel in focus: the parameters are rtHipDepthOfFieldLens's for the scene's camera and that pixel's depth
        depth = rs.readback_passes()["depth"]
        ys, xs = np.nonzero(np.isfinite(depth))
        x, y = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])
        got = rs.depth_of_field(aperture=0.05, focus_pixel=(x, y), rings=2)
        focus, scale = DO.lens(rs.camera(), 0.05, depth[y, x])
        assert F32(got["params"]["focus"]).tobytes() == focus.tobytes() == depth[y, x].tobytes()
        assert F32(got["params"]["coc_scale"]).tobytes() == scale.tobytes() and got["params"]["rings"] == 2
        assert_same(got["rgb"], DO.blur(frame_colour(rs), depth, **got["params"]), "lens")
        if (~np.isfinite(depth)).any():
            ys, xs = np.nonzero(~np.isfinite(depth))
            with pytest.raises(ValueError, match="hit nothing"):
                rs.depth_of_field(aperture=0.05, focus_pixel=(int(xs[0]), int(ys[0])))
        with pytest.raises(ValueError):
            rs.depth_of_field(aperture=0.05, focus_pixel=(sc.width, 0))
    finally:
        rs.close()


def test_the_scene_path_on_four_scene_tiles_equals_the_oracle():
    """axis_near_axis_mixed at 136 x 132: 2 x 2 scene tiles of 128 pixels, the right-hand and the lower ones partly filled, so the scene
    gather runs with slot > 0 and tilesX > 1; 5 x 5 blur tiles, so interior ones exist."""
    name = "axis_near_axis_mixed"
    sc = MC.base_scene(name, MC.CAMERA_SCENES[name])
    assert R.tile_count(sc.width, sc.height) == 4 and sc.width > 128 and sc.height > 128
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(depth=True)
        for pose in ("home", "pan"):
            if pose != "home":
                move(rs, MC.posed(sc, pose))
            share = dof_step(rs, f"{name}/{pose}")
            assert share >= DC.MIN_GATHER, (pose, share)
            # the blur reaches more than one scene tile: pixels of several 128 x 128 tiles differ from the frame
            colour, depth = frame_colour(rs), rs.readback_passes()["depth"]
            for params in SCENE_PARAMS:
                out = DO.blur(colour, depth, focus=focus_of(depth), **params)
                changed = ~DO.same_bits(out, colour).all(-1)
                tiles = {(int(y) // 128, int(x) // 128) for y, x in zip(*np.nonzero(changed))}
                assert len(tiles) > 1, (pose, params, tiles)
    finally:
        rs.close()


def test_the_call_leaves_the_scene_as_a_twin_that_never_calls_and_makes_its_storage_once():
    sc = MC.base_scene(SCENE, SIZE)
    twin, rs = R.ResidentScene(sc, 0), R.ResidentScene(sc, 0)
    params = dict(focus=2.0, **SCENE_PARAMS[0])

    def products(s):
        """Everything a later frame shows of the state the call must not touch."""
        acc = s.temporal()  # (marks)
        flow = s.motion()
        passes = s.readback_passes()
        return ([p.copy() for p in s.readback()] + [passes["depth"], passes["alpha"], passes["triangle"], acc["colour"], acc["count"]]
                + [flow[k] for k in ("motion", "t", "prev_t", "triangle")] + [np.concatenate([v.ravel() for v in s.motion_reference_camera().values() if hasattr(v, "ravel")])])

    try:
        for s in (twin, rs):
            s.set_passes(alpha=True, depth=True, triangle=True)
            s.render()
            s.temporal()
        bytes0 = rs.bytes()
        assert twin.bytes() == bytes0
        frame, passes = [p.copy() for p in rs.readback()], rs.readback_passes()
        first = rs.depth_of_field(**params)
        grown = rs.bytes()
        n = sc.width * sc.height
        part = lambda b: (b + 255) // 256 * 256  # noqa: E731
        assert grown - bytes0 == (2 * part(n * 12) + part(n * 4) + 3 * part(n * 2)
                                  + part(R.lib().rtHipDepthOfFieldScratchBytes(sc.width, sc.height)))
        second = rs.depth_of_field(**params)
        assert rs.bytes() == grown  # the second call makes nothing more
        assert_same(second["rgb"], first["rgb"], "the second call")
        assert not np.array_equal(first["rgb"], frame_colour(rs))  # (it did blur)
        assert all(np.array_equal(a, b) for a, b in zip(rs.readback(), frame))  # the tile buffer is what it was
        again = rs.readback_passes()
        assert all(np.array_equal(again[k], passes[k], equal_nan=k == "depth") for k in ("alpha", "depth", "triangle"))  # and the passes
        only = R.lib().rtHipSceneDepthOfField(rs.handle, C.byref(R.dof_params(**params)), None, None, None, None)  # every output left out
        assert only == 0
        assert twin.bytes() == bytes0  # a scene that never calls is the size it was
        for pose in ("pan", "orbit90"):  # the next frames, their accumulation and their flow: bit-identical to the twin's
            for s in (twin, rs):
                move(s, MC.posed(sc, pose))
                s.render()
            rs.depth_of_field(**params)
            for i, (a, b) in enumerate(zip(products(twin), products(rs))):
                assert a.tobytes() == b.tobytes(), (pose, i)
    finally:
        rs.close()
        twin.close()


def test_scene_refusals_launch_nothing():
    sc = MC.base_scene("axis_near_axis_mixed", MC.CAMERA_SCENES["axis_near_axis_mixed"])  # several tiles
    L = R.lib()
    H, W = sc.height, sc.width
    rgb = np.full((H, W, 3), -7.0, F32)
    planes = [np.full((H, W), 12345, np.uint16) for _ in range(3)]

    def call(rs, params=None):
        return L.rtHipSceneDepthOfField(rs.handle, C.byref(params or R.dof_params()), *[a.ctypes.data_as(C.c_void_p) for a in [rgb] + planes])

    tiles = np.arange(R.tile_count(W, H), dtype=np.uint32)
    for part in (tiles[1:], np.concatenate([tiles, tiles[:1]])):
        rs = R.ResidentScene(sc, 0, part)
        try:
            rs.set_passes(depth=True)
            rs.render()
            bytes0 = rs.bytes()
            assert call(rs) == -1 and "every tile of the image" in R.last_error()
            with pytest.raises(RuntimeError, match="every tile of the image"):
                rs.depth_of_field()
            assert rs.bytes() == bytes0
        finally:
            rs.close()
    rs = R.ResidentScene(sc, 0)
    try:
        rs.render()
        bytes0 = rs.bytes()
        assert call(rs) == -1 and "depth pass" in R.last_error()  # no pass at all
        rs.set_passes(alpha=True, triangle=True)  # the pass buffer is there, the depth bit is not
        rs.render()
        bytes0 = rs.bytes()
        assert call(rs) == -1 and "depth pass" in R.last_error()
        with pytest.raises(RuntimeError, match="depth pass"):
            rs.depth_of_field(focus_pixel=(0, 0))
        rs.set_passes(depth=True)
        rs.render()
        bytes0 = rs.bytes()
        for bad, word in ((dict(focus=0.0), "focus"), (dict(coc_scale=-1.0), "cocScale"), (dict(max_coc=0.5), "maxCoc"), (dict(rings=0), "rings"),
                          (dict(rings=7), "rings"), (dict(depth_softness=-1.0), "depthSoftness")):
            assert call(rs, R.dof_params(**bad)) == -1 and word in R.last_error(), bad
            assert rs.bytes() == bytes0
    finally:
        rs.close()
    assert (rgb == -7.0).all() and all((p == 12345).all() for p in planes)


def test_command_line_writes_what_the_api_returns(tmp_path):
    from opencl_render_amd import __main__ as M
    args = ["--scene", "soup", "--width", "64", "--height", "48", "--samples", "1", "--triangles", "20000", "--out", str(tmp_path / "img.bmp")]
    assert M.main(args + ["--dof", str(tmp_path / "one.pfm"), "--aperture", "0.02", "--focus", "3.0", "--dof-rings", "2", "--max-coc", "9"]) == 0
    sc = S.make_soup(64, 48, 20000, 0.02, samples=1)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(depth=True)
        hit = np.ones((48, 64), bool)  # a pixel whose ray hits something in both views of the orbit
        for position in R.orbit_positions(np.zeros(3, F32), np.float32([0, 0, 3]), 2):
            rs.look_at(position, np.float32([0, 0, 3]), (0, 1, 0), np.radians(M.parser().get_default("fov")))
            rs.render()
            hit &= np.isfinite(rs.readback_passes()["depth"])
        assert hit.any(), "no pixel of the soup is hit in both views"
        py, px = (int(v[0]) for v in np.nonzero(hit))
        assert M.main(args + ["--orbit", "2", "--dof", str(tmp_path / "dof.ppm"), "--aperture", "0.5", "--focus-pixel", str(px), str(py)]) == 0
    finally:
        rs.close()
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(depth=True)
        rs.render()
        want = rs.depth_of_field(aperture=0.02, focus=3.0, rings=2, max_coc=9.0)
        assert open(tmp_path / "one.pfm", "rb").read() == b"PF\n64 48\n-1.0\n" + want["rgb"][::-1].astype("<f4").tobytes()
        blurred = 0
        for i, position in enumerate(R.orbit_positions(np.zeros(3, F32), np.float32([0, 0, 3]), 2)):
            rs.look_at(position, np.float32([0, 0, 3]), (0, 1, 0), np.radians(M.parser().get_default("fov")))
            rs.render()
            want = rs.depth_of_field(aperture=0.5, focus_pixel=(px, py))
            blurred += int(not np.array_equal(want["rgb"], frame_colour(rs)))
            F.write_ppm(str(tmp_path / "want.ppm"), *want["planes"])
            assert open(tmp_path / f"dof_{i:03d}.ppm", "rb").read() == open(tmp_path / "want.ppm", "rb").read(), i
        assert blurred == 2  # (both views were blurred: the files are not the frames)
    finally:
        rs.close()
    for bad in (["--dof", str(tmp_path / "d.pfm")], ["--dof", str(tmp_path / "d.pfm"), "--aperture", "0.1"],
                ["--dof", str(tmp_path / "d.png"), "--aperture", "0.1", "--focus", "1"], ["--aperture", "0.1"],
                ["--dof", str(tmp_path / "d.pfm"), "--aperture", "0.1", "--focus", "1", "--focus-pixel", "1", "1"],
                ["--dof", str(tmp_path / "d.pfm"), "--aperture", "0.1", "--focus", "1", "--dof-rings", "7"],
                ["--dof", str(tmp_path / "d.pfm"), "--aperture", "0.1", "--focus", "1", "--max-coc", "33"]):
        with pytest.raises(SystemExit):
            M.parse_args(bad)
