"""Render passes on the MI355X (run with -m gpu): alpha / depth / triangle from the wavefront pipeline's primary stage against an
expectation computed here from the scene's camera lists, in numpy float32 with the oracle's generator and triangle test; the beauty
image left untouched; sample batching, planned frames, tile sets, the megakernel guard, the buffer's lifetime and the command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import scenarios
from conftest import ROOT, golden_names, load_golden_scene
from opencl_render_amd import frontend as F, raytrace as R

pytestmark = pytest.mark.gpu

ALL = dict(alpha=True, depth=True, triangle=True)


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the render pass tests cannot run (and the product has no CPU fallback)")


def expected_passes(sc):
    """alpha, depth, triangle as the definitions have them: sample s of pixel p = y*W + x draws from seed p*S + s (LR jitter, then TB),
    tests the pixel's camera list in order with a running closest hit (ties keep the earlier candidate)."""
    L = O.oracle()
    f3 = C.c_float * 3
    W, H, S = sc.width, sc.height, sc.sample_count
    eye = f3(*[float(v) for v in sc.eye[:3]])
    tl, lr, tb = (np.asarray(v, np.float32)[:3] for v in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    verts = [[f3(*[float(c) for c in sc.vertex[int(i)][:3]]) for i in sc.tri_index[t][:3]] for t in range(sc.triangle_count)]
    alpha = np.zeros((H, W), np.uint16)
    depth = np.full((H, W), np.inf, np.float32)
    tri = np.full((H, W), 0xFFFFFFFF, np.uint32)
    t, l1, l2 = C.c_float(), C.c_float(), C.c_float()
    for y in range(H):
        for x in range(W):
            p = y * W + x
            cands = [int(c) for c in sc.cam_list[int(sc.cam_start[p]):int(sc.cam_end[p])]]
            hits = 0
            for s in range(1, S + 1):
                state = C.c_uint64(p * S + s)
                kx = np.float32(x) + np.float32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
                ky = np.float32(y) + np.float32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
                d = tl.copy()
                d = d + lr * kx
                d = d + tb * ky
                dc = f3(*[float(v) for v in d])
                best, best_t = None, np.float32(np.inf)
                for c in cands:
                    a, b, cc = verts[c]
                    if L.rt_oracle_ray_triangle(eye, dc, 0.0, float(best_t), a, b, cc, C.byref(t), C.byref(l1), C.byref(l2)):
                        best, best_t = c, np.float32(t.value)
                hits += best is not None
                if s == 1 and best is not None:
                    tri[y, x] = best
                    depth[y, x] = best_t * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            alpha[y, x] = hits * 65535 // S
    return dict(alpha=alpha, depth=depth, triangle=tri)


_expected = {}


def expected(name):
    if name not in _expected:
        sc, _ = load_golden_scene(name)
        _expected[name] = expected_passes(sc)
    return _expected[name]


def assert_passes(got, want, what):
    for k in ("alpha", "triangle"):
        bad = int((got[k] != want[k]).sum())
        assert bad == 0, f"{what}: pass {k} differs in {bad}/{want[k].size} pixels"
    bad = int((got["depth"].view(np.uint32) != want["depth"].view(np.uint32)).sum())
    assert bad == 0, f"{what}: pass depth differs bitwise in {bad}/{want['depth'].size} pixels"


def render_passes(sc, tiles=None, **passes):
    rs = R.ResidentScene(sc, 0, tiles)
    try:
        rs.set_passes(**(passes or ALL))
        rs.render()
        planes = rs.readback()
        return planes, rs.readback_passes()
    finally:
        rs.close()


@pytest.mark.parametrize("name", golden_names())
def test_passes_match_the_definition_and_leave_the_image_alone(name):
    sc, want_planes = load_golden_scene(name)
    planes, got = render_passes(sc)
    assert_passes(got, expected(name), name)
    tri = got["triangle"]
    hit = tri != 0xFFFFFFFF
    assert np.array_equal(got["material"][hit], sc.tri_material[tri[hit]]) and (got["material"][~hit] == -1).all()
    assert "mesh" not in got  # (a golden scene is not made of front-end meshes)
    for ch, g, w in zip("RGB", planes, want_planes):
        assert np.array_equal(g.reshape(w.shape), w), f"{name}: plane {ch} changed with the passes on"


def test_sample_batches_do_not_change_the_passes(monkeypatch):
    sc, want_planes = load_golden_scene("sparse_many_samples")  # 80x60, S=5
    for mb in ("20", "40"):  # ~1 and ~2 samples per batch for one 128x128 tile
        monkeypatch.setenv("RT_WF_STATE_MB", mb)
        planes, got = render_passes(sc)
        assert_passes(got, expected("sparse_many_samples"), f"state budget {mb} MB")
        for g, w in zip(planes, want_planes):
            assert np.array_equal(g.reshape(w.shape), w)
    monkeypatch.delenv("RT_WF_STATE_MB")


def test_a_planned_frame_gives_the_same_passes():
    sc, _ = load_golden_scene("sparse_many_samples")
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(**ALL)
        rs.render()
        first = {k: v.copy() for k, v in rs.readback_passes().items()}
        rs.render()  # planned: no host synchronisation; its hit counters must start from zero again
        second = rs.readback_passes()
    finally:
        rs.close()
    assert_passes(first, expected("sparse_many_samples"), "first frame")
    assert_passes(second, first, "second (planned) frame")


def test_disjoint_tile_sets_compose():
    sc, _ = load_golden_scene("odd_size_multi_tile")
    whole = render_passes(sc)[1]
    tiles = np.arange(R.tile_count(sc.width, sc.height), dtype=np.uint32)
    parts = None
    for sub in (tiles[0::2], tiles[1::2]):
        rs = R.ResidentScene(sc, 0, sub)
        try:
            rs.set_passes(**ALL)
            rs.render()
            parts = rs.readback_passes(parts)
        finally:
            rs.close()
    assert_passes(parts, whole, "two instances")
    assert_passes(whole, expected("odd_size_multi_tile"), "one instance")


def test_shuffled_partial_tiles_land_where_they_belong():
    """Slot order that is not image order, one slot mostly outside the image: the instance's pixels are the whole image's, bit for bit,
    and the pixels of other tiles keep what the arrays held."""
    sc, tiles = scenarios.shuffled_tiles(), scenarios.SHUFFLED_TILES
    whole, part = render_passes(sc)[1], render_passes(sc, tiles)[1]
    mine = scenarios.tiles_mask(sc, tiles)
    assert (whole["alpha"][128:, 128:] != 0).any() and (whole["alpha"][:128, :128] != 0).any()  # both tiles show something
    assert_passes({k: v[mine] for k, v in part.items()}, {k: v[mine] for k, v in whole.items()}, "tiles 3, 0")
    assert (part["alpha"][~mine] == 0).all() and np.isinf(part["depth"][~mine]).all() and (part["triangle"][~mine] == 0xFFFFFFFF).all()


def test_megakernel_is_refused_and_passes_off_frees_the_buffer():
    sc, _ = load_golden_scene("primary_only")
    rs = R.ResidentScene(sc, 0)
    try:
        base = rs.bytes()
        assert rs.pass_buffer() == (None, 0)
        rs.set_passes(alpha=True)
        ptr, nbytes = rs.pass_buffer()
        assert ptr and nbytes == len(rs.tiles) * 3 * 128 * 128 * 4 and rs.bytes() == base + nbytes
        with pytest.raises(RuntimeError, match="render passes"):
            rs.set_pipeline(R.PIPELINE_MEGAKERNEL)
        depth = np.zeros(sc.pixels, np.float32)  # a pass the scene does not have
        assert R.lib().rtHipReadbackPasses(rs.handle, None, depth.ctypes.data_as(C.c_void_p), None) != 0
        assert "depth pass is not on" in R.last_error()
        rs.set_passes()
        assert rs.pass_buffer() == (None, 0) and rs.bytes() == base
        rs.set_pipeline(R.PIPELINE_MEGAKERNEL)
        with pytest.raises(RuntimeError, match="megakernel"):
            rs.set_passes(triangle=True)
        rs.set_pipeline(R.PIPELINE_WAVEFRONT)
        rs.set_passes(alpha=True)  # alpha only: the others are not returned
        rs.render()
        got = rs.readback_passes()
        assert sorted(got) == ["alpha"] and np.array_equal(got["alpha"], expected("primary_only")["alpha"])
    finally:
        rs.close()


def test_command_line_writes_the_passes(tmp_path):
    prefix = str(tmp_path / "frame")
    obj = os.path.join(ROOT, "tests", "data", "scene.obj")
    args = ["--obj", obj, "--width", "96", "--height", "64", "--samples", "3", "--out", str(tmp_path / "img.ppm"), "--passes", prefix]
    run = subprocess.run([sys.executable, "-m", "opencl_render_amd"] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    # the same scene, built the way the command line builds it, through readback_passes
    mesh, materials = F.read_obj(obj)
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    centre, size = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) or 1.0
    sc = F.scene_from_meshes([mesh], materials, [dict(type=3, dir=(0.3, -0.8, 0.5))], centre + np.float32([0.35, 0.25, -1.0]) * size, centre,
                             (0, 1, 0), np.radians(50.0), 96, 64, samples=3)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    _, want = render_passes(sc)
    assert set(np.unique(want["mesh"])) <= {-1, 0}  # one mesh
    pgm = open(prefix + "_alpha.pgm", "rb").read()
    assert pgm == b"P5\n96 64\n255\n" + (want["alpha"] >> 8).astype(np.uint8).tobytes()
    pfm = open(prefix + "_depth.pfm", "rb").read()
    assert pfm == b"Pf\n96 64\n-1.0\n" + want["depth"][::-1].astype("<f4").tobytes()
    ids = np.load(prefix + "_ids.npz")
    for k in ("triangle", "material", "mesh"):
        assert np.array_equal(ids[k], want[k]), k
    assert (want["alpha"] > 0).any()
