"""Ambient occlusion on the MI355X (run with -m gpu): rtHipSceneAmbientOcclusion / rtHipSceneAmbientOcclusionDevice give, bit for bit,
the image of the numpy restatement (ao_oracle.py, walks by rt_oracle_grid_trace) on every golden scene and the AXIS scenes over
R in {1, 5, 16}, Sp in {1, 3}, an infinite and a short radius and two seeds, at the edges R = 256 and Sp = 64, and on a 1M-triangle
soup at 1080p against the image assembled from ResidentScene.intersect; host and device entry points, numpy and torch agree; instances
over a tile deal compose and leave other pixels alone; frames around an AO call are unchanged; refusals launch nothing; --ao writes
what the API returns."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest
import torch  # (before the library loads its HIP runtime: the order bench.py uses)

import ao_oracle as A
import scenarios
from conftest import golden_names, load_golden_scene
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the ambient occlusion tests cannot run (and the product has no CPU fallback)")


def crop(sc, w, h):
    """The central w x h window of sc's image (the same camera, its top-left moved to the window's), camera lists rebuilt."""
    if sc.width <= w and sc.height <= h:
        return sc
    w, h = min(w, sc.width), min(h, sc.height)
    x0, y0 = (sc.width - w) // 2, (sc.height - h) // 2
    tl = np.asarray(sc.eye_to_top_left, F32).copy()
    lr, tb = np.asarray(sc.left_to_right, F32), np.asarray(sc.top_to_bottom, F32)
    tl[:3] = (tl[:3] + lr[:3] * F32(x0)) + tb[:3] * F32(y0)
    out = dataclasses.replace(sc, width=w, height=h, eye_to_top_left=tl, cam_start=None, cam_end=None, cam_list=None)
    R.build_camera_list(out, threads=16)
    return out


def short_radius(sc):
    b = np.asarray(sc.box_min, np.float64)
    return float(0.02 * np.linalg.norm(b[256, :3] - b[0, :3]))


def device_ao(sc, **kw):
    rs = R.ResidentScene(sc)
    try:
        return rs.ambient_occlusion(**kw)
    finally:
        rs.close()


def assert_bits(got, want, what):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} pixels differ; first {bad[:4]}: got {got.ravel()[bad[:4]]}, want {want.ravel()[bad[:4]]}"


# R x Sp x radius x seed: 24 combinations, dealt over the golden and AXIS scenes in turn
COMBOS = list(itertools.product((1, 5, 16), (1, 3), ("inf", "short"), (0, 0x9E3779B9)))
SCENES = [("golden", n) for n in golden_names()] + [("axis", f.__name__) for f in scenarios.AXIS]


@pytest.mark.parametrize("i", range(len(SCENES)), ids=[n for _, n in SCENES])
def test_bit_exact_against_the_oracle(i):
    kind, name = SCENES[i]
    sc = load_golden_scene(name)[0] if kind == "golden" else scenarios.axis_by_name(name)()
    if name == "odd_size_multi_tile":  # several tiles, one of them partly outside the image
        sc, combos = crop(sc, 136, 132), [(1, 1, "short", 5)]
    else:
        sc, combos = crop(sc, 24, 16), [COMBOS[i % len(COMBOS)], COMBOS[(i + 12) % len(COMBOS)]]
    for rays, sp, rad, seed in combos:
        radius = np.inf if rad == "inf" else short_radius(sc)
        want = A.ambient_occlusion(sc, rays=rays, radius=radius, pixel_samples=sp, seed=seed)
        got = device_ao(sc, rays=rays, radius=radius, pixel_samples=sp, seed=seed)
        assert_bits(got, want, f"{name} R={rays} Sp={sp} radius={rad} seed={seed}")
        assert ((want >= 0) & (want <= 1)).all()


def test_edges_of_the_parameter_ranges():
    base = load_golden_scene("lambert_distant")[0]
    for (w, h), rays, sp in (((8, 6), 256, 1), ((8, 6), 1, 64), ((2, 2), 256, 64)):
        sc = crop(base, w, h)
        want = A.ambient_occlusion(sc, rays=rays, pixel_samples=sp, seed=3)
        assert_bits(device_ao(sc, rays=rays, pixel_samples=sp, seed=3), want, f"{w}x{h} R={rays} Sp={sp}")


def test_small_chunks_give_the_same_image():
    sc = crop(load_golden_scene("mixed_materials_textured")[0], 24, 16)
    want = device_ao(sc, rays=5, pixel_samples=3, seed=1)
    R.tune("ao_samples", 77)  # pixel samples of one pixel split over chunks
    try:
        assert_bits(device_ao(sc, rays=5, pixel_samples=3, seed=1), want, "77-sample chunks")
    finally:
        R.tune("reset", 0)


def test_million_triangle_soup_at_1080p_against_intersect():
    sc = S.make_soup(1920, 1080, 1_000_000, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc)
    try:
        got = rs.ambient_occlusion(rays=4, seed=2)

        def walk(rays):
            return rs.intersect(rays["o"], rays["d"], rays["tmin"], rays["tmax"], rays["excluded"])

        want, rays = A.ambient_occlusion(sc, rays=4, seed=2, walk=walk, with_rays=True)
    finally:
        rs.close()
    assert len(rays["sample"]) > 0.2 * 4 * sc.pixels  # hits: the image is not just misses
    assert 0.05 < float(want.mean()) < 0.999
    assert_bits(got, want, "soup_1m 1080p R=4")


@pytest.fixture(scope="module")
def axis_scene():
    return crop(scenarios.axis_by_name("axis_near_axis_mixed")(), 40, 30)


def test_host_device_numpy_torch_agree(axis_scene):
    sc = axis_scene
    kw = dict(rays=5, pixel_samples=3, radius=short_radius(sc), seed=11)
    want = A.ambient_occlusion(sc, **kw)
    rs = R.ResidentScene(sc)
    dev = torch.device("cuda", 0)
    try:
        host = rs.ambient_occlusion(**kw)
        assert_bits(host, want, "host entry")
        out = torch.full((sc.height, sc.width), -1.0, device=dev)
        assert rs.ambient_occlusion(out=out, **kw) is out
        torch.cuda.synchronize()
        assert_bits(out.cpu().numpy(), want, "device entry (torch, current stream)")
        side = torch.cuda.Stream(dev)  # a foreign stream, and twice on it: the scratch is reused in order
        out2 = torch.zeros_like(out)
        with torch.cuda.stream(side):
            rs.ambient_occlusion(out=out2, **kw)
            rs.ambient_occlusion(out=out2, **kw)
        torch.cuda.synchronize()
        assert_bits(out2.cpu().numpy(), want, "device entry (foreign stream)")
        nump = np.full((sc.height, sc.width), 5.0, F32)
        assert rs.ambient_occlusion(out=nump, **kw) is nump
        assert_bits(nump, want, "host entry into out")
        with pytest.raises(ValueError):
            rs.ambient_occlusion(out=torch.zeros((sc.height, sc.width + 1), device=dev))
        with pytest.raises(ValueError):
            rs.ambient_occlusion(out=np.zeros((sc.height, sc.width), np.float64))
    finally:
        rs.close()


def test_instances_over_a_tile_deal_compose():
    sc = crop(load_golden_scene("odd_size_multi_tile")[0], 200, 150)
    kw = dict(rays=3, pixel_samples=1, seed=4)
    full = device_ao(sc, **kw)
    dev = torch.device("cuda", 0)
    parts, host, devout = [], np.full((sc.height, sc.width), -7.0, F32), torch.full((sc.height, sc.width), -7.0, device=dev)
    try:
        for rank in range(2):
            tiles = R.tiles_of_rank(sc.width, sc.height, rank, 2)
            parts.append(R.ResidentScene(sc, 0, tiles, like=parts[0] if parts else None))
            parts[-1].ambient_occlusion(out=host, **kw)
            parts[-1].ambient_occlusion(out=devout, **kw)
            torch.cuda.synchronize()
            if rank == 0:  # only this instance's tiles are written
                mine = np.zeros((sc.height, sc.width), bool)
                for t in tiles:
                    ty, tx = divmod(int(t), (sc.width + R.TILE - 1) // R.TILE)
                    mine[ty * R.TILE:(ty + 1) * R.TILE, tx * R.TILE:(tx + 1) * R.TILE] = True
                assert (host[~mine] == -7.0).all() and (devout.cpu().numpy()[~mine] == -7.0).all()
                assert_bits(host[mine], full[mine], "rank 0's tiles")
    finally:
        for p in parts:
            p.close()
    assert_bits(host, full, "two instances composed (host)")
    assert_bits(devout.cpu().numpy(), full, "two instances composed (device)")


def test_host_and_device_entries_agree_on_shuffled_partial_tiles():
    """Slot order that is not image order, one slot mostly outside the image: the host entry point's image is the device entry point's,
    bit for bit, other tiles' pixels left alone by both."""
    sc, tiles = scenarios.shuffled_tiles(), scenarios.SHUFFLED_TILES
    kw = dict(rays=3, pixel_samples=2, seed=6)
    host = np.full((sc.height, sc.width), -7.0, F32)
    devout = torch.full((sc.height, sc.width), -7.0, device=torch.device("cuda", 0))
    rs = R.ResidentScene(sc, 0, tiles)
    try:
        rs.ambient_occlusion(out=host, **kw)
        rs.ambient_occlusion(out=devout, **kw)
        torch.cuda.synchronize()
    finally:
        rs.close()
    mine = scenarios.tiles_mask(sc, tiles)
    assert_bits(host, devout.cpu().numpy(), "tiles 3, 0")
    assert (host[~mine] == -7.0).all() and ((host[mine] >= 0) & (host[mine] <= 1)).all() and (host[mine] < 1).any()


def test_frames_around_an_ao_call_are_unchanged():
    sc = load_golden_scene("lambert_distant")[0]
    rs = R.ResidentScene(sc)
    try:
        rs.set_passes(alpha=True, depth=True, triangle=True, normal=True, albedo=True)
        rs.render()
        planes = rs.readback()
        passes = rs.readback_passes()
        before = rs.bytes()
        rs.ambient_occlusion(rays=16, pixel_samples=3, seed=1)
        assert rs.bytes() > before  # the scratch is counted
        rs.render()
        assert all(np.array_equal(a, b) for a, b in zip(planes, rs.readback()))
        again = rs.readback_passes()
        for k in passes:
            assert np.array_equal(np.asarray(passes[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8)), k
    finally:
        rs.close()


def test_refusals_return_minus_one_and_launch_nothing(axis_scene):
    sc = axis_scene
    L = R.lib()
    rs = R.ResidentScene(sc)
    dev = torch.device("cuda", 0)
    try:
        out = torch.full((sc.height, sc.width), -3.0, device=dev)
        host = np.full((sc.height, sc.width), -3.0, F32)
        ptr = C.c_void_p(out.data_ptr())
        good = R.ao_params()
        bad = [R.ao_params(rays=r) for r in (0, 257)] + [R.ao_params(pixel_samples=s) for s in (0, 65)] + \
              [R.ao_params(radius=r) for r in (0.0, -1.0, float("nan"), -float("inf"))]
        for p in bad:
            assert L.rtHipSceneAmbientOcclusionDevice(rs.handle, C.byref(p), ptr, None) == -1
            assert L.rtHipSceneAmbientOcclusion(rs.handle, C.byref(p), host.ctypes.data_as(C.c_void_p)) == -1
            assert R.last_error()
        assert L.rtHipSceneAmbientOcclusionDevice(None, C.byref(good), ptr, None) == -1
        assert L.rtHipSceneAmbientOcclusionDevice(rs.handle, None, ptr, None) == -1
        assert L.rtHipSceneAmbientOcclusionDevice(rs.handle, C.byref(good), None, None) == -1
        assert L.rtHipSceneAmbientOcclusion(rs.handle, C.byref(good), None) == -1
        assert L.rtHipSceneAmbientOcclusionDevice(rs.handle, C.byref(good), host.ctypes.data_as(C.c_void_p), None) == -1
        assert "not device memory" in R.last_error()
        torch.cuda.synchronize()
        assert (out == -3.0).all() and (host == -3.0).all()
        with pytest.raises(RuntimeError):
            rs.ambient_occlusion(rays=0)
    finally:
        rs.close()


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1]


def read_pgm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        w, h = (int(v) for v in f.readline().split())
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(), np.uint8).reshape(h, w)


def test_command_line_writes_pfm_and_pgm(tmp_path):
    from opencl_render_amd import __main__ as M
    args = ["--scene", "soup", "--width", "64", "--height", "48", "--samples", "1", "--triangles", "20000", "--out", str(tmp_path / "img.bmp"),
            "--ao-rays", "6", "--ao-samples", "2", "--ao-seed", "9", "--ao-radius", "0.3"]
    assert M.main(args + ["--ao", str(tmp_path / "ao.pfm")]) == 0
    assert M.main(args + ["--ao", str(tmp_path / "ao.pgm")]) == 0
    sc = S.make_soup(64, 48, 20000, 0.02, samples=1)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    want = device_ao(sc, rays=6, pixel_samples=2, seed=9, radius=0.3)
    assert (want < 1).any() and (want == 1).any()
    assert_bits(np.ascontiguousarray(read_pfm(tmp_path / "ao.pfm")), want, "--ao .pfm")
    u16 = R.quantise(want[..., None].repeat(3, -1))[0]
    assert np.array_equal(read_pgm(tmp_path / "ao.pgm"), (u16 >> 8).astype(np.uint8))
    with pytest.raises(SystemExit):
        M.parse_args(["--ao", str(tmp_path / "ao.png")])
