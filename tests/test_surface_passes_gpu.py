"""Surface passes on the MI355X (run with -m gpu): the shading normal and the albedo at the primary hit, means over a pixel's samples,
against the definition of include/raytrace_hip.h computed here with the oracle's generator, triangle test, shading normal and texel
look-up, summed in numpy float32 in sample order; the beauty image and the other passes left untouched; sample batching, planned
frames, tile sets, the buffers' lifetime and guards, a 1080p frame and the command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import scenarios as SC
from conftest import ROOT, golden_names, load_golden_scene
from opencl_render_amd import frontend as F, raytrace as R, scene as S

pytestmark = pytest.mark.gpu

BASIC = dict(alpha=True, depth=True, triangle=True)
SURFACE = dict(normal=True, albedo=True)
ALL = dict(BASIC, **SURFACE)
SCENARIOS = ["class_textured_bumped"]  # one-texel height maps: no golden scene has one


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the surface pass tests cannot run (and the product has no CPU fallback)")


def surface_definition(sc, pixels=None):
    """normal, albedo [H, W, 3] f32 as the header defines them (only the flat pixel indices `pixels` when given; the others stay 0), and
    what the hit samples covered: sample s of pixel p draws from seed p*S + s (LR jitter, then TB) and scans the pixel's camera list in
    order with a running closest hit; a hit adds GetTriangleNormal at where = eye + t*dir and the colour channel's texel, a miss adds 0;
    the sums are taken in float32 in sample order and divided by float32(S)."""
    L = O.oracle()
    fp = C.POINTER(C.c_float)
    L.rt_oracle_shading_normal.argtypes = [C.POINTER(O.OracleScene), fp, fp, fp, C.c_uint32, C.c_float, C.c_float, fp]
    dummy = [np.zeros(1, np.uint16) for _ in range(3)]
    osc = O.oracle_scene(sc, dummy)
    f3 = C.c_float * 3
    W, H, S_ = sc.width, sc.height, sc.sample_count
    eye = np.asarray(sc.eye, np.float32)[:3]
    eye_c = f3(*[float(v) for v in eye])
    tl, lr, tb = (np.asarray(v, np.float32)[:3] for v in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    verts = {}

    def tri_verts(t):
        if t not in verts:
            verts[t] = [f3(*[float(c) for c in sc.vertex[int(i)][:3]]) for i in sc.tri_index[t][:3]]
        return verts[t]

    mat_size = np.asarray(sc.mat_size, np.uint32).reshape(-1, 2)
    tri_uv = np.ascontiguousarray(sc.tri_uv, np.float32).reshape(-1, 6)
    normal = np.zeros((H * W, 3), np.float32)
    albedo = np.zeros((H * W, 3), np.float32)
    seen = dict(material_none=0, colour_image=0, bump_image=0, bump_one_texel=0, mixed_pixels=0, hit_samples=0)
    t, l1, l2 = C.c_float(), C.c_float(), C.c_float()
    n_out = np.zeros(3, np.float32)
    a_out = np.zeros(3, np.float32)
    for p in (range(H * W) if pixels is None else pixels):
        p = int(p)
        x, y = p % W, p // W
        cands = [int(c) for c in sc.cam_list[int(sc.cam_start[p]):int(sc.cam_end[p])]]
        acc_n = np.zeros(3, np.float32)
        acc_a = np.zeros(3, np.float32)
        hits = 0
        for s in range(1, S_ + 1):
            state = C.c_uint64(p * S_ + s)
            kx = np.float32(x) + np.float32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
            ky = np.float32(y) + np.float32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
            d = tl.copy()
            d = d + lr * kx
            d = d + tb * ky
            dc = f3(*[float(v) for v in d])
            best, best_t, best_l1, best_l2 = None, np.float32(np.inf), 0.0, 0.0
            for c in cands:
                a, b, cc = tri_verts(c)
                if L.rt_oracle_ray_triangle(eye_c, dc, 0.0, float(best_t), a, b, cc, C.byref(t), C.byref(l1), C.byref(l2)):
                    best, best_t, best_l1, best_l2 = c, np.float32(t.value), l1.value, l2.value
            n_s = np.zeros(3, np.float32)
            a_s = np.zeros(3, np.float32)
            if best is not None:
                hits += 1
                where = eye + best_t * d  # per component in float32: eye + t*dir (along())
                L.rt_oracle_shading_normal(C.byref(osc), where.ctypes.data_as(fp), eye.ctypes.data_as(fp), d.ctypes.data_as(fp), best,
                                           best_l1, best_l2, n_out.ctypes.data_as(fp))
                n_s = n_out.copy()
                m = int(sc.tri_material[best])
                if m < 0:
                    seen["material_none"] += 1
                else:
                    cw, ch = (int(v) for v in mat_size[S.CH_COUNT * m + S.CH_COLOR])
                    bw, bh = (int(v) for v in mat_size[S.CH_COUNT * m + S.CH_BUMP])
                    seen["colour_image"] += cw * ch > 1
                    seen["bump_image"] += bw * bh > 1
                    seen["bump_one_texel"] += bw == 1 and bh == 1
                    if cw > 0:
                        table = sc.textures[int(sc.mat_start[S.CH_COUNT * m + S.CH_COLOR]):]
                        L.rt_oracle_texel(table.ctypes.data_as(C.c_void_p), cw, ch, tri_uv[best].ctypes.data_as(fp), best_l1, best_l2,
                                          a_out.ctypes.data_as(fp))
                        a_s = a_out.copy()
            acc_n = acc_n + n_s
            acc_a = acc_a + a_s
        seen["hit_samples"] += hits
        seen["mixed_pixels"] += 0 < hits < S_
        normal[p] = acc_n / np.float32(S_)
        albedo[p] = acc_a / np.float32(S_)
    return dict(normal=normal.reshape(H, W, 3), albedo=albedo.reshape(H, W, 3)), seen


def scene_of(name):
    """A golden scene (and its stored planes) or a scenario scene built here (planes None)."""
    if name in SCENARIOS:
        sc = SC.class_by_name(name)()
        R.build_lists(sc)
        return sc, None
    return load_golden_scene(name)


_expected = {}


def expected(name):
    if name not in _expected:
        _expected[name] = surface_definition(scene_of(name)[0])
    return _expected[name]


def same_bits(got, want):
    """Rows (pixels) that differ by bit pattern; any NaN equals any NaN (payloads are not pinned between x86 and gfx950)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    eq = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return np.flatnonzero(~eq.reshape(-1, 3).all(1))


def assert_surface(got, want, what, pixels=None):
    for k in ("normal", "albedo"):
        g, w = got[k].reshape(-1, 3), want[k].reshape(-1, 3)
        if pixels is not None:
            g, w = g[pixels], w[pixels]
        bad = same_bits(g, w)
        assert bad.size == 0, f"{what}: pass {k} differs in {bad.size}/{len(w)} pixels, first {bad[0]}: {g[bad[0]]} vs {w[bad[0]]}"


def render(sc, tiles=None, **passes):
    rs = R.ResidentScene(sc, 0, tiles)
    try:
        rs.set_passes(**passes)
        rs.render()
        planes = [p.copy() for p in rs.readback()]
        return planes, rs.readback_passes()
    finally:
        rs.close()


@pytest.mark.parametrize("name", golden_names() + SCENARIOS)
def test_surface_passes_match_the_definition_and_leave_the_rest_alone(name):
    sc, want_planes = scene_of(name)
    planes, got = render(sc, **ALL)
    assert sorted(got) == ["albedo", "alpha", "depth", "material", "normal", "triangle"]
    assert got["normal"].shape == (sc.height, sc.width, 3) and got["normal"].dtype == np.float32
    assert_surface(got, expected(name)[0], name)
    basic_planes, basic = render(sc, **BASIC)
    for k in ("alpha", "depth", "triangle", "material"):
        assert basic[k].tobytes() == got[k].tobytes(), f"{name}: pass {k} changed when NORMAL|ALBEDO were added"
    if want_planes is None:
        want_planes = render(sc)[0]
    for ch, g, b, w in zip("RGB", planes, basic_planes, want_planes):
        assert np.array_equal(g.reshape(w.shape), w), f"{name}: plane {ch} changed with the surface passes on"
        assert np.array_equal(b.reshape(w.shape), w)


def test_the_scenes_cover_every_kind_of_surface():
    seen = {}
    for name in golden_names() + SCENARIOS:
        for k, v in expected(name)[1].items():
            seen[k] = seen.get(k, 0) + v
    for k in ("material_none", "colour_image", "bump_image", "bump_one_texel", "mixed_pixels"):
        assert seen[k] > 0, f"no hit sample of kind {k} in the scenes: {seen}"


def test_sample_batches_do_not_change_the_surface_passes(monkeypatch):
    sc, want_planes = load_golden_scene("sparse_many_samples")  # 80x60, S=5
    for mb in ("20", "40"):  # ~1 and ~2 samples per batch for one 128x128 tile
        monkeypatch.setenv("RT_WF_STATE_MB", mb)
        planes, got = render(sc, **SURFACE)
        assert_surface(got, expected("sparse_many_samples")[0], f"state budget {mb} MB")
        for g, w in zip(planes, want_planes):
            assert np.array_equal(g.reshape(w.shape), w)
    monkeypatch.delenv("RT_WF_STATE_MB")


def test_a_planned_frame_gives_the_same_surface_passes():
    sc, _ = load_golden_scene("sparse_many_samples")
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(**SURFACE)
        rs.render()
        first = {k: v.copy() for k, v in rs.readback_passes().items()}
        rs.render()  # planned: no host synchronisation; its first batch must start the sums from zero again
        second = rs.readback_passes()
    finally:
        rs.close()
    assert_surface(first, expected("sparse_many_samples")[0], "first frame")
    assert_surface(second, first, "second (planned) frame")


def test_disjoint_tile_sets_compose():
    sc, _ = load_golden_scene("odd_size_multi_tile")
    whole = render(sc, **ALL)[1]
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
    assert_surface(parts, whole, "two instances")
    assert_surface(whole, expected("odd_size_multi_tile")[0], "one instance")


def test_shuffled_partial_tiles_land_where_they_belong():
    """Slot order that is not image order, one slot mostly outside the image: the instance's pixels are the whole image's, bit for bit,
    and the pixels of other tiles keep what the arrays held."""
    sc, tiles = SC.shuffled_tiles(), SC.SHUFFLED_TILES
    whole, part = render(sc, **ALL)[1], render(sc, tiles, **ALL)[1]
    mine = SC.tiles_mask(sc, tiles)
    assert whole["normal"][128:, 128:].any() and whole["normal"][:128, :128].any()  # both tiles show something
    assert_surface(part, whole, "tiles 3, 0", pixels=np.flatnonzero(mine.reshape(-1)))
    assert not part["normal"][~mine].any() and not part["albedo"][~mine].any()


def test_buffers_live_while_their_passes_are_on_and_the_guards_hold():
    sc, _ = load_golden_scene("primary_only")
    rs = R.ResidentScene(sc, 0)
    surface_bytes = len(rs.tiles) * 6 * 128 * 128 * 4
    pass_bytes = len(rs.tiles) * 3 * 128 * 128 * 4
    try:
        base = rs.bytes()
        assert rs.surface_buffer() == (None, 0)
        with pytest.raises(RuntimeError, match="unknown render pass bits"):
            rs._check(R.lib().rtHipScenePasses(rs.handle, 32), "rtHipScenePasses")
        rs.set_passes(normal=True)  # normal only: the surface buffer, not the pass buffer
        ptr, nbytes = rs.surface_buffer()
        assert ptr and nbytes == surface_bytes and rs.bytes() == base + surface_bytes
        assert rs.pass_buffer() == (None, 0)
        with pytest.raises(RuntimeError, match="render passes"):
            rs.set_pipeline(R.PIPELINE_MEGAKERNEL)
        rs.render()
        got = rs.readback_passes()
        assert sorted(got) == ["normal"]
        assert_surface(dict(got, albedo=expected("primary_only")[0]["albedo"]), expected("primary_only")[0], "normal only")
        albedo = np.zeros(sc.pixels * 3, np.float32)  # a pass the scene does not have
        assert R.lib().rtHipReadbackSurfacePasses(rs.handle, None, albedo.ctypes.data_as(C.c_void_p)) != 0
        assert "albedo pass is not on" in R.last_error()
        rs.set_passes(alpha=True, albedo=True)  # both buffers
        assert rs.pass_buffer()[1] == pass_bytes and rs.surface_buffer()[1] == surface_bytes
        assert rs.bytes() == base + pass_bytes + surface_bytes
        rs.set_passes(alpha=True)  # the surface buffer goes, the pass buffer stays
        assert rs.surface_buffer() == (None, 0) and rs.pass_buffer()[1] == pass_bytes and rs.bytes() == base + pass_bytes
        normal = np.zeros(sc.pixels * 3, np.float32)
        assert R.lib().rtHipReadbackSurfacePasses(rs.handle, normal.ctypes.data_as(C.c_void_p), None) != 0
        assert "normal pass is not on" in R.last_error()
        rs.set_passes(albedo=True)
        rs.set_passes()  # mask 0 frees both
        assert rs.surface_buffer() == (None, 0) and rs.pass_buffer() == (None, 0) and rs.bytes() == base
        rs.set_pipeline(R.PIPELINE_MEGAKERNEL)
        with pytest.raises(RuntimeError, match="megakernel"):
            rs.set_passes(albedo=True)
        assert rs.surface_buffer() == (None, 0)
    finally:
        rs.close()


@pytest.mark.parametrize("samples", [1, 4])
def test_a_1080p_million_triangle_frame_matches_the_definition(samples):
    w = dict(width=1920, height=1080, triangles=1_000_000, edge=0.004)  # bench.py's lambert_1m
    sc = S.make_soup(w["width"], w["height"], w["triangles"], w["edge"], seed=12345, samples=samples, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    _, got = render(sc, **ALL)
    rng = np.random.Generator(np.random.PCG64(samples))
    covered = np.flatnonzero(got["alpha"].ravel() > 0)
    pixels = np.unique(np.concatenate([rng.choice(sc.pixels, 200, replace=False), rng.choice(covered, 200, replace=False)]))
    want, seen = surface_definition(sc, pixels)
    assert seen["hit_samples"] > 0
    assert_surface(got, want, f"1080p S={samples}", pixels)


def test_command_line_writes_the_surface_passes(tmp_path):
    obj = os.path.join(ROOT, "tests", "data", "scene.obj")

    def run(prefix, *extra):
        args = ["--obj", obj, "--width", "96", "--height", "64", "--samples", "3", "--out", str(tmp_path / "img.ppm"), "--passes", prefix]
        done = subprocess.run([sys.executable, "-m", "opencl_render_amd"] + args + list(extra), cwd=ROOT, capture_output=True, text=True,
                              timeout=300)
        assert done.returncode == 0, done.stderr

    (tmp_path / "with").mkdir()
    (tmp_path / "without").mkdir()
    run(str(tmp_path / "with" / "frame"), "--surface-passes")
    run(str(tmp_path / "without" / "frame"))
    assert sorted(os.listdir(tmp_path / "without")) == ["frame_alpha.pgm", "frame_depth.pfm", "frame_ids.npz"]
    assert sorted(os.listdir(tmp_path / "with")) == ["frame_albedo.pfm", "frame_alpha.pgm", "frame_depth.pfm", "frame_ids.npz",
                                                     "frame_normal.pfm"]
    # the same scene, built the way the command line builds it, through readback_passes
    mesh, materials = F.read_obj(obj)
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    centre, size = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) or 1.0
    sc = F.scene_from_meshes([mesh], materials, [dict(type=3, dir=(0.3, -0.8, 0.5))], centre + np.float32([0.35, 0.25, -1.0]) * size, centre,
                             (0, 1, 0), np.radians(50.0), 96, 64, samples=3)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    _, want = render(sc, **ALL)
    for k in ("normal", "albedo"):
        pfm = open(tmp_path / "with" / f"frame_{k}.pfm", "rb").read()
        assert pfm == b"PF\n96 64\n-1.0\n" + want[k][::-1].astype("<f4").tobytes(), k
    assert (np.abs(want["normal"]).sum(-1) > 0).any() and (want["albedo"].sum(-1) > 0).any()
    for k in ("alpha.pgm", "depth.pfm"):
        assert open(tmp_path / "with" / f"frame_{k}", "rb").read() == open(tmp_path / "without" / f"frame_{k}", "rb").read(), k
