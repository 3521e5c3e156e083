"""The denoiser on the MI355X (run with -m gpu): the device output against tests/denoise_oracle.py bit for bit, the host and device entry
points, the device entry's pointer checks, the scene path (rtHipSceneDenoise) against the oracle fed the host read-backs, its guards and
scratch lifetime, composition over a tile deal, the image quality on the demo room and the command line's --denoise."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the library loads its HIP runtime: the order bench.py uses)

import denoise_oracle as D
import scenarios as SC
from conftest import ROOT, golden_names, load_golden_scene
from opencl_render_amd import demo, frontend as F, raytrace as R

pytestmark = pytest.mark.gpu

SURFACE = dict(normal=True, albedo=True)
SCENARIOS = ["class_textured_bumped"]
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (127, 129), (128, 128), (333, 200)]  # (W, H)
PARAMS = {
    "default": {},
    "no_edge_stops": dict(colour_inv_sigma2=0.0, albedo_inv_sigma2=0.0),
    "sharp": dict(colour_inv_sigma2=1e6, albedo_inv_sigma2=1e5, normal_power_log2=10),
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the denoiser tests cannot run (and the product has no CPU fallback)")


def inputs(W, H, seed):
    """Seeded colour, normal and albedo with bands of zero, subnormal-length and random-length normals and of zero albedo."""
    rng = np.random.default_rng(seed)
    colour = rng.random((H, W, 3), dtype=np.float32)
    normal = (rng.standard_normal((H, W, 3)) * rng.choice([1e-3, 1.0, 1e3], (H, W, 1))).astype(np.float32)
    albedo = rng.random((H, W, 3), dtype=np.float32)
    band = (np.arange(H)[:, None] + 2 * np.arange(W)[None, :]) % 7
    normal[band == 0] = 0.0
    normal[band == 1] = (rng.standard_normal(((band == 1).sum(), 3)) * 1e-21).astype(np.float32)  # m is subnormal or underflows
    albedo[band == 2] = 0.0
    normal[band == 3] = [0.0, 0.0, 1.0]  # flat patches: wn near 1, so colour edges decide
    return colour, normal, albedo


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(-1, 3).any(1))
    assert bad.size == 0, f"{what}: {bad.size}/{want.size // 3} pixels differ, first {bad[0]}: {got.reshape(-1, 3)[bad[0]]} vs {want.reshape(-1, 3)[bad[0]]}"


def on_gpu(*arrays):
    return [torch.from_numpy(a).to("cuda:0") for a in arrays]


@pytest.mark.parametrize("W, H", SIZES)
@pytest.mark.parametrize("K", [0, 1, 2, 5, 8])
def test_device_output_matches_the_oracle_bit_for_bit(W, H, K):
    c, n, a = inputs(W, H, 100 * W + H + K)
    for name, extra in PARAMS.items():
        if name != "default" and K not in (2, 5):
            continue
        want = D.denoise(c, n, a, **dict(R.DENOISE_DEFAULTS, iterations=K, **extra))
        got = R.denoise(*on_gpu(c, n, a), iterations=K, **extra)
        torch.cuda.synchronize()
        same_bits(got.cpu().numpy(), want, f"{W}x{H} K={K} {name}")
        if K == 0:
            assert got.cpu().numpy().tobytes() == c.tobytes()


def test_a_1080p_frame_matches_the_oracle_bit_for_bit():
    c, n, a = inputs(1920, 1080, 7)
    want = D.denoise(c, n, a, iterations=2)
    got = R.denoise(*on_gpu(c, n, a), iterations=2)
    torch.cuda.synchronize()
    same_bits(got.cpu().numpy(), want, "1920x1080 K=2")


def test_host_and_device_entry_points_agree():
    for (W, H), K in (((127, 129), 5), ((333, 200), 8)):
        c, n, a = inputs(W, H, W * H)
        host = R.denoise(c, n, a, iterations=K)
        dev = R.denoise(*on_gpu(c, n, a), iterations=K)
        torch.cuda.synchronize()
        assert host.tobytes() == dev.cpu().numpy().tobytes()


def test_the_device_entry_refuses_bad_pointers_and_launches_nothing():
    W, H = 37, 23
    img = W * H * 12
    L = R.lib()
    need = L.rtHipDenoiseScratchBytes(W, H)
    c, n, a = inputs(W, H, 3)
    made = []

    def alloc(nbytes, data=None):  # exact allocations, so that a range past their end is seen
        ptr = L.rtHipDeviceAlloc(0, nbytes)
        assert ptr, R.last_error()
        made.append(ptr)
        if data is not None:
            assert L.rtHipDeviceCopy(0, C.c_void_p(ptr), data.ctypes.data_as(C.c_void_p), data.nbytes, 1) == 0
        return ptr

    try:
        dc, dn, da = alloc(img, c), alloc(img, n), alloc(img, a)
        sentinel = np.full((H, W, 3), 7.0, np.float32)
        out, scratch = alloc(img, sentinel), alloc(need)
        p = R.denoise_params()

        def call(colour=dc, normal=dn, albedo=da, dst=out, scr=scratch, nbytes=need):
            return L.rtHipDenoiseDevice(0, W, H, C.c_void_p(colour), C.c_void_p(normal), C.c_void_p(albedo), C.c_void_p(dst),
                                        C.c_void_p(scr), nbytes, C.byref(p), None)

        host = np.zeros((H, W, 3), np.float32)
        assert call(colour=host.ctypes.data) == -1 and "colour" in R.last_error() and "not device memory" in R.last_error()
        assert call(dst=host.ctypes.data) == -1 and "not device memory" in R.last_error()
        assert call(normal=alloc(img - 4)) == -1 and "reach past the end" in R.last_error()
        assert call(scr=alloc(need - 16)) == -1 and "reach past the end" in R.last_error()
        assert call(nbytes=need - 1) == -1 and "scratch of" in R.last_error()
        assert call(dst=dc) == -1 and "overlaps colour" in R.last_error()
        assert call(dst=da + 12) == -1 and "overlaps albedo" in R.last_error()
        both = alloc(img + need)
        assert call(dst=both, scr=both + img - 16) == -1 and "overlaps" in R.last_error()
        assert call(scr=dn) == -1 and "overlaps normal" in R.last_error()
        assert call(scr=alloc(need + 4) + 4) == -1 and "aligned" in R.last_error()
        got = np.zeros_like(sentinel)
        assert L.rtHipDeviceCopy(0, got.ctypes.data_as(C.c_void_p), C.c_void_p(out), img, 0) == 0
        assert got.tobytes() == sentinel.tobytes(), "a refused call wrote its output"
        assert call() == 0
        assert L.rtHipDeviceCopy(0, got.ctypes.data_as(C.c_void_p), C.c_void_p(out), img, 0) == 0  # (synchronises the device)
        same_bits(got, D.denoise(c, n, a), "after the refusals")
    finally:
        for ptr in made:
            L.rtHipDeviceFree(0, C.c_void_p(ptr))


def test_the_device_entry_takes_a_stream_of_its_device_only():
    c, n, a = inputs(64, 48, 9)
    want = D.denoise(c, n, a)
    side = torch.cuda.Stream(device=0)
    with torch.cuda.stream(side):  # a stream that is not the null stream
        got = R.denoise(*on_gpu(c, n, a))
    side.synchronize()
    same_bits(got.cpu().numpy(), want, "on a side stream")
    if torch.cuda.device_count() > 1:  # a stream of device 1 for a call on device 0
        other = torch.cuda.Stream(device=1)
        tc, tn, ta = on_gpu(c, n, a)
        out = torch.empty_like(tc)
        nbytes = R.lib().rtHipDenoiseScratchBytes(64, 48)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        rc = R.lib().rtHipDenoiseDevice(0, 64, 48, *[C.c_void_p(t.data_ptr()) for t in (tc, tn, ta, out, scratch)], nbytes,
                                        C.byref(R.denoise_params()), C.c_void_p(other.cuda_stream))
        assert rc == -1 and "belongs to device 1" in R.last_error()


def scene_of(name):
    if name in SCENARIOS:
        sc = SC.class_by_name(name)()
        R.build_lists(sc)
        return sc
    return load_golden_scene(name)[0]


def render(sc, tiles=None, **passes):
    rs = R.ResidentScene(sc, 0, tiles)
    rs.set_passes(**passes)
    rs.render()
    return rs


def oracle_of(rs, **params):
    sc = rs.scene
    planes = [p.reshape(sc.height, sc.width).copy() for p in rs.readback()]
    surf = rs.readback_passes()
    colour, normal, albedo = D.inputs(planes, surf["normal"], surf["albedo"])
    want = D.denoise(colour, normal, albedo, **dict(R.DENOISE_DEFAULTS, **params))
    return want, planes, surf


@pytest.mark.parametrize("name", golden_names() + SCENARIOS)
def test_scene_denoise_matches_the_oracle_on_the_read_backs(name):
    sc = scene_of(name)
    rs = render(sc, **SURFACE)
    try:
        for params in ({}, dict(iterations=3, colour_inv_sigma2=0.5, normal_power_log2=2)):
            want, _, _ = oracle_of(rs, **params)
            got = rs.denoise(**params)
            assert got["colour"].shape == (sc.height, sc.width, 3) and got["colour"].dtype == np.float32
            same_bits(got["colour"], want, f"{name} {params}")
            for ch, g, w in zip("RGB", got["planes"], D.quantise(want)):
                assert g.dtype == np.uint16 and np.array_equal(g, w), f"{name} {params}: plane {ch}"
    finally:
        rs.close()


def test_scene_denoise_changes_neither_the_frame_nor_the_next_one():
    sc = load_golden_scene("odd_size_multi_tile")[0]
    rs = render(sc, alpha=True, depth=True, triangle=True, **SURFACE)
    try:
        before = [p.copy() for p in rs.readback()]
        passes = {k: v.copy() for k, v in rs.readback_passes().items()}
        first = rs.denoise()
        assert all(np.array_equal(p, q) for p, q in zip(rs.readback(), before))
        after = rs.readback_passes()
        assert all(after[k].tobytes() == passes[k].tobytes() for k in passes)
        rs.render()
        assert all(np.array_equal(p, q) for p, q in zip(rs.readback(), before))
        assert all(rs.readback_passes()[k].tobytes() == passes[k].tobytes() for k in passes)
        assert rs.denoise()["colour"].tobytes() == first["colour"].tobytes()
    finally:
        rs.close()


def test_scene_denoise_guards_and_scratch_lifetime():
    sc = load_golden_scene("primary_only")[0]
    rs = R.ResidentScene(sc, 0)
    try:
        base = rs.bytes()
        rs.render()
        with pytest.raises(RuntimeError, match="normal and the albedo pass"):
            rs.denoise()
        for one in (dict(normal=True), dict(albedo=True), dict(normal=True, alpha=True)):
            rs.set_passes(**one)
            rs.render()
            with pytest.raises(RuntimeError, match="normal and the albedo pass"):
                rs.denoise()
        rs.set_passes(**SURFACE)
        rs.render()
        with_surface = rs.bytes()
        assert rs.denoise_times_ms() == dict(gather=0.0, prologue=0.0, filter=0.0)
        rs.denoise()
        times = rs.denoise_times_ms()
        assert all(v > 0 for v in times.values()), times
        n = sc.width * sc.height
        assert rs.bytes() > with_surface + 64 * n  # the scene's scratch is counted
        again = rs.bytes()
        rs.denoise(iterations=2)
        assert rs.bytes() == again  # made once
        with pytest.raises(RuntimeError, match="iterations 13"):
            rs.denoise(iterations=13)
        rs.set_passes(normal=True)  # the denoiser cannot run: its scratch goes
        assert rs.bytes() == base + rs.surface_buffer()[1]
        rs.set_passes(**SURFACE)
        rs.render()
        rs.denoise()
        rs.set_passes()
        assert rs.bytes() == base
    finally:
        rs.close()
    sc = load_golden_scene("odd_size_multi_tile")[0]
    tiles = np.arange(R.tile_count(sc.width, sc.height), dtype=np.uint32)
    for part in (tiles[1:], np.concatenate([tiles, tiles[:1]])):
        rs = render(sc, part, **SURFACE)
        try:
            with pytest.raises(RuntimeError, match="every tile of the image"):
                rs.denoise()
        finally:
            rs.close()


def test_two_instances_composed_on_the_host_equal_one_scene():
    sc = load_golden_scene("odd_size_multi_tile")[0]
    whole = render(sc, **SURFACE)
    try:
        want = whole.denoise()
    finally:
        whole.close()
    tiles = np.arange(R.tile_count(sc.width, sc.height), dtype=np.uint32)
    planes = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
    passes = None
    for sub in (tiles[0::2], tiles[1::2]):
        rs = render(sc, sub, **SURFACE)
        try:
            rs.readback(planes)
            passes = rs.readback_passes(passes)
        finally:
            rs.close()
    colour, normal, albedo = D.inputs([p.reshape(sc.height, sc.width) for p in planes], passes["normal"], passes["albedo"])
    got = R.denoise(colour, normal, albedo, device=0)
    assert got.tobytes() == want["colour"].tobytes()
    assert all(np.array_equal(g, w) for g, w in zip(R.quantise(got), want["planes"]))


def test_denoising_brings_a_two_sample_room_much_closer_to_the_converged_one():
    W, H = 320, 240

    def frame(samples):
        sc = demo.room_scene(W, H, samples=samples)
        R.build_lists(sc)
        rs = render(sc, **SURFACE)
        try:
            colour = np.stack([p.reshape(H, W) for p in rs.readback()], -1).astype(np.float32) / np.float32(65535)
            return colour, rs.denoise()["colour"]
        finally:
            rs.close()

    truth, _ = frame(256)
    noisy, denoised = frame(2)
    mse_noisy = float(np.mean((noisy.astype(np.float64) - truth) ** 2))
    mse_denoised = float(np.mean((denoised.astype(np.float64) - truth) ** 2))
    print(f"room {W}x{H} S=2 vs S=256: MSE noisy {mse_noisy:.3e}, denoised {mse_denoised:.3e}, ratio {mse_noisy / mse_denoised:.2f}")
    assert mse_denoised * 8.0 < mse_noisy  # measured: 12.6 (MSE 5.08e-3 noisy, 4.02e-4 denoised)


def test_command_line_writes_the_denoised_frame(tmp_path):
    W, H, S = 96, 64, 3
    args = ["--scene", "room", "--width", str(W), "--height", str(H), "--samples", str(S), "--out", str(tmp_path / "noisy.ppm")]
    for ext in ("ppm", "pfm"):
        done = subprocess.run([sys.executable, "-m", "opencl_render_amd"] + args + ["--denoise", str(tmp_path / f"den.{ext}")], cwd=ROOT,
                              capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stderr
    sc = demo.room_scene(W, H, samples=S)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = render(sc, **SURFACE)
    try:
        want, planes, _ = oracle_of(rs)
    finally:
        rs.close()
    F.write_ppm(str(tmp_path / "want.ppm"), *D.quantise(want))
    F.write_ppm(str(tmp_path / "want_noisy.ppm"), *planes)
    assert open(tmp_path / "den.ppm", "rb").read() == open(tmp_path / "want.ppm", "rb").read()
    assert open(tmp_path / "noisy.ppm", "rb").read() == open(tmp_path / "want_noisy.ppm", "rb").read()
    assert open(tmp_path / "den.pfm", "rb").read() == b"PF\n%d %d\n-1.0\n" % (W, H) + want[::-1].astype("<f4").tobytes()
    assert not np.array_equal(D.quantise(want)[0], planes[0])
