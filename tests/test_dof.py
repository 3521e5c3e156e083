"""Depth of field without a GPU: the C ABI declares and exports the entry points and refuses NULL arguments and parameters out of range, at
their legal edges too; the kernel's per-pixel code (csrc/rt_dof_pixel.h) compiled for the host equals the numpy restatement
(dof_oracle.py) bit for bit over every case of dof_cases.py; the lens helper equals its float64 restatement; the restatement has the
properties a depth of field must have -- no aperture or nothing out of focus copies the frame, a constant colour stays, a sharp pixel
stays sharp in front of a blurred background, the background's blur ends at maxCoc, an isolated pixel spreads over its own disc --; and
the inputs of tests/test_dof_gpu.py are not vacuous.  The device is checked against the same restatement there."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dof_cases as DC
import dof_oracle as DO
from conftest import ROOT
from opencl_render_amd import raytrace as R

F32 = np.float32
ENTRY_POINTS = ("rtHipDepthOfFieldCheck", "rtHipDepthOfFieldDevice", "rtHipDepthOfField", "rtHipSceneDepthOfField",
                "rtHipSceneDepthOfFieldTimes", "rtHipDepthOfFieldLens")


def test_header_declares_the_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert re.search(r"\bvoid\s+rtHipDepthOfFieldDefaults\s*\(", text) and hasattr(hip_lib, "rtHipDepthOfFieldDefaults")
    assert re.search(r"\buint64_t\s+rtHipDepthOfFieldScratchBytes\s*\(", text) and hasattr(hip_lib, "rtHipDepthOfFieldScratchBytes")
    assert text.index("MOTION BLUR:") < text.index("DEPTH OF FIELD:") < text.index("AMBIENT OCCLUSION BAKE:")
    block = text[text.index("DEPTH OF FIELD:"):text.index("AMBIENT OCCLUSION BAKE:")]
    for word in ("Not done", "axial depth", "lens sampling", "anti-aliased depth", "in-painting", "bokeh", "tile-dealt", "sphere"):
        assert word in block, word
    for method in ("depth_of_field", "depth_of_field_times_ms"):
        assert callable(getattr(R.ResidentScene, method))
    assert callable(R.depth_of_field) and callable(R.dof_params)
    assert C.sizeof(R.DofParams) == 20
    assert [f[0] for f in R.DofParams._fields_] == ["focus", "cocScale", "maxCoc", "rings", "depthSoftness"]
    p = R.DofParams()
    hip_lib.rtHipDepthOfFieldDefaults(C.byref(p))
    assert (p.focus, p.cocScale, p.maxCoc, p.rings, p.depthSoftness) == (F32(1.0), F32(8.0), F32(16.0), 3, F32(0.05))
    assert R.DEPTH_OF_FIELD_DEFAULTS == dict(focus=1.0, coc_scale=8.0, max_coc=16.0, rings=3, depth_softness=0.05) == DO.DEFAULTS
    assert hip_lib.rtHipDepthOfFieldCheck(C.byref(p)) == 0


def test_parameter_refusals_and_their_legal_edges(hip_lib):
    check = lambda **kw: hip_lib.rtHipDepthOfFieldCheck(C.byref(R.dof_params(**kw)))  # noqa: E731
    assert hip_lib.rtHipDepthOfFieldCheck(None) == -1 and "null parameters" in R.last_error()
    assert check() == 0
    up = lambda v, to=np.inf: np.nextafter(F32(v), F32(to))  # noqa: E731
    edges = (dict(focus=DC.DENORMAL), dict(focus=3e38), dict(focus=np.finfo(F32).max), dict(coc_scale=0.0), dict(coc_scale=-0.0),
             dict(coc_scale=DC.DENORMAL), dict(coc_scale=4096.0), dict(max_coc=1.0), dict(max_coc=32.0), dict(rings=1), dict(rings=6),
             dict(depth_softness=0.0), dict(depth_softness=3e38))
    for good in edges:
        assert check(**good) == 0, good
    refused = (("focus", dict(focus=0.0)), ("focus", dict(focus=-0.0)), ("focus", dict(focus=-DC.DENORMAL)), ("focus", dict(focus=np.nan)),
               ("focus", dict(focus=np.inf)), ("focus", dict(focus=-1.0)),
               ("cocScale", dict(coc_scale=-DC.DENORMAL)), ("cocScale", dict(coc_scale=up(4096.0))), ("cocScale", dict(coc_scale=np.nan)),
               ("cocScale", dict(coc_scale=np.inf)), ("cocScale", dict(coc_scale=-np.inf)),
               ("maxCoc", dict(max_coc=up(1.0, 0.0))), ("maxCoc", dict(max_coc=up(32.0))), ("maxCoc", dict(max_coc=0.0)),
               ("maxCoc", dict(max_coc=np.nan)), ("maxCoc", dict(max_coc=np.inf)),
               ("rings", dict(rings=0)), ("rings", dict(rings=7)), ("rings", dict(rings=0xFFFFFFFF)),
               ("depthSoftness", dict(depth_softness=-DC.DENORMAL)), ("depthSoftness", dict(depth_softness=np.nan)),
               ("depthSoftness", dict(depth_softness=np.inf)))
    for word, bad in refused:
        assert check(**bad) == -1 and word in R.last_error(), bad
    with pytest.raises(ValueError):
        R.dof_params(rings=-1)


def test_null_arguments_bad_parameters_bad_sizes_and_a_short_scratch_are_refused_without_a_device(hip_lib):
    """(Nothing here reaches a device: the parameters, the sizes, the NULL checks and the scratch size come first.)"""
    L = hip_lib
    W, H = 4, 3
    f = [np.full((H, W, 3), -3.0, F32) for _ in range(4)]
    ptr = [a.ctypes.data_as(C.c_void_p) for a in f]
    good = R.dof_params()
    assert L.rtHipSceneDepthOfField(None, C.byref(good), ptr[0], None, None, None) == -1 and "null" in R.last_error()
    assert L.rtHipSceneDepthOfFieldTimes(None, (C.c_float * 3)()) == -1 and "null" in R.last_error()
    calls = ((lambda a, p, w=W, h=H: L.rtHipDepthOfField(0, w, h, *a[:3], p), 3),
             (lambda a, p, w=W, h=H: L.rtHipDepthOfFieldDevice(0, w, h, *a[:4], 1 << 20, p, None), 4))
    for call, arrays in calls:
        assert call(ptr, None) == -1 and "null parameters" in R.last_error()
        for i in range(arrays):
            args = list(ptr)
            args[i] = None
            assert call(args, C.byref(good)) == -1 and "null array" in R.last_error(), i
        assert call(ptr, C.byref(R.dof_params(rings=0))) == -1 and "rings" in R.last_error()
        for w, h in ((0, 3), (4, 0), (16385, 1), (1, 16385), (16384, 16384)):
            assert call(ptr, C.byref(good), w, h) == -1 and "image" in R.last_error(), (w, h)
    need = L.rtHipDepthOfFieldScratchBytes(W, H)
    assert L.rtHipDepthOfFieldDevice(0, W, H, *ptr[:4], need - 1, C.byref(good), None) == -1 and "scratch" in R.last_error()
    assert str(need) in R.last_error()
    assert all((a == -3.0).all() for a in f)
    with pytest.raises(ValueError):
        R.depth_of_field(f[0], f[1])  # a depth array of three channels


def test_the_scratch_formula(hip_lib):
    L = hip_lib
    assert L.rtHipDepthOfFieldScratchBytes(0, 3) == 0 and L.rtHipDepthOfFieldScratchBytes(16385, 1) == 0
    assert L.rtHipDepthOfFieldScratchBytes(16384, 16384) == 0
    up16 = lambda b: (b + 15) // 16 * 16  # noqa: E731
    for W, H in DC.SHAPES + (DC.WIDE, DC.INTERIOR, DC.TALL, (1920, 1080), (16384, 8192)):
        tiles = ((W + 31) // 32) * ((H + 31) // 32)
        assert L.rtHipDepthOfFieldScratchBytes(W, H) == up16(W * H * 8) + 2 * up16(tiles * 4), (W, H)
    assert L.rtHipDepthOfFieldScratchBytes(33, 33) == 8720 + 2 * 16


# ---- the kernel's per-pixel code, compiled for the host ---------------------------------------------------------------------------------
HOST_FLAGS = ["-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]  # csrc/Makefile's exactness flags


@pytest.fixture(scope="module")
def host_blur(tmp_path_factory):
    """tests/dof_host.cpp (csrc/rt_dof_pixel.h, with a sequential (b) and (c)) as a host library."""
    out = tmp_path_factory.mktemp("dof_host") / "libdof_host.so"
    subprocess.run([os.environ.get("CXX", "g++")] + HOST_FLAGS + ["-I", os.path.join(ROOT, "opencl_render_amd", "csrc"), "-o", str(out),
                    os.path.join(ROOT, "tests", "dof_host.cpp")], check=True)
    lib = C.CDLL(str(out))
    lib.dof_host.restype = None
    lib.dof_host.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_float]

    def run(colour, depth, focus, coc_scale, max_coc, rings, depth_softness):
        H, W = depth.shape
        out = np.full((H, W, 3), -7.0, F32)
        lib.dof_host(W, H, colour.ctypes.data, depth.ctypes.data, out.ctypes.data, focus, coc_scale, max_coc, rings, depth_softness)
        return out

    return run


@pytest.mark.parametrize("name, W, H", DC.CASES)
def test_the_kernels_pixel_code_on_the_host_equals_the_oracle_bit_for_bit(host_blur, name, W, H):
    fields = DC.fields(name, W, H)
    for params in DC.grid_of(W, H):
        want, got = DC.reference(name, W, H, params), host_blur(*fields, **params)
        bad = np.flatnonzero(~DO.same_bits(got, want).reshape(-1))
        assert bad.size == 0, f"{name} {W}x{H} {params}: differs in {bad.size} values, first {bad[:4]}"


def test_every_shape_field_and_grid_value_is_among_the_cases():
    assert {(W, H) for _, W, H in DC.CASES} == set(DC.SHAPES) | {DC.WIDE, DC.INTERIOR, DC.TALL}
    assert {name for name, _, _ in DC.CASES} == set(DC.FIELDS)
    assert all(DC.grid_of(W, H) is (DC.ORDINARY if (W, H) == DC.TALL else DC.GRID) for _, W, H in DC.CASES)
    assert {n for n, W, H in DC.CASES if (W, H) == DC.INTERIOR} == {"layers", "near_sharp"}
    assert {n for n, W, H in DC.CASES if (W, H) == DC.TALL} == {"ramp", "layers"}
    for key, values in (("rings", range(1, 7)), ("max_coc", (1.0, 32.0)), ("coc_scale", (0.0, DC.DENORMAL, 4096.0)),
                        ("focus", (DC.DENORMAL, 3e38)), ("depth_softness", (0.0, 3e38))):
        assert set(values) <= {p[key] for p in DC.GRID}, key
    assert len(DC.EXTREMES) == 6 * 2 * 3 * 2 * 2 and F32(DC.DENORMAL).view(np.uint32) == 1
    assert all(R.lib().rtHipDepthOfFieldCheck(C.byref(R.dof_params(**p))) == 0 for p in DC.GRID)
    _, z = DC.fields("specials", 64, 40)
    assert np.isnan(z).any() and (z == 0).any() and (z == -1).any() and (z == -np.inf).any() and (z == F32(DC.DENORMAL)).any()
    assert (z == F32(3e38)).any() and (z == np.inf).any()
    c, _ = DC.fields("specials", 64, 40)
    assert np.isnan(c).any() and (c == F32(3e38)).any()


# ---- the lens helper ------------------------------------------------------------------------------------------------------------------
def call_lens(camera, aperture, focus, start):
    cam = R.Camera()
    for dst, key in ((cam.eyeToTopLeft, "eye_to_top_left"), (cam.leftToRight, "left_to_right"), (cam.topToBottom, "top_to_bottom")):
        for i in range(4):
            dst[i] = camera[key][i] if i < 3 else np.nan  # (lane 3 is never read)
    p = R.dof_params(**start)
    return R.lib().rtHipDepthOfFieldLens(C.byref(cam), aperture, focus, C.byref(p)), p


def test_the_lens_helper_equals_its_float64_restatement_bit_for_bit_and_refuses_degenerate_cameras(hip_lib):
    start = dict(focus=7.0, coc_scale=5.0, max_coc=9.0, rings=2, depth_softness=0.25)
    filled = refused = 0
    for name, vectors in DC.LENS_CAMERAS.items():
        camera = DC.camera_dict(vectors)
        for aperture, focus in DC.LENS_SETTINGS:
            want = DO.lens(camera, aperture, focus)
            rc, p = call_lens(camera, aperture, focus, start)
            if want is None:
                refused += 1
                assert rc == -1 and R.last_error(), (name, aperture, focus)
                assert (p.focus, p.cocScale) == (F32(7.0), F32(5.0))  # unchanged
            else:
                filled += 1
                assert rc == 0, (name, aperture, focus, R.last_error())
                assert F32(p.focus).tobytes() == want[0].tobytes() and F32(p.cocScale).tobytes() == want[1].tobytes(), (name, aperture, focus)
            assert (p.maxCoc, p.rings, p.depthSoftness) == (F32(9.0), 2, F32(0.25))  # the other fields are kept
    assert filled >= 9 and refused >= 3  # (a result out of range is refused: cocScale above 4096, a focus that rounds to nothing)
    fp = DO.focal_pixels(*(np.asarray(v, F32) for v in DC.LENS_CAMERAS["soup"]))[0]
    assert abs(fp - 1920.0) < 1e-3  # the soups' camera: the plane at distance 1, 1920 pixels across a width of 1
    for name, vectors in DC.LENS_DEGENERATE.items():
        assert DO.lens(DC.camera_dict(vectors), 0.01, 4.0) is None, name
        rc, p = call_lens(DC.camera_dict(vectors), 0.01, 4.0, start)
        assert rc == -1 and "camera" in R.last_error() and (p.focus, p.cocScale) == (F32(7.0), F32(5.0)), name
    good = DC.camera_dict(DC.LENS_CAMERAS["soup"])
    for aperture, focus in ((0.01, 0.0), (0.01, -1.0), (0.01, np.nan), (0.01, np.inf), (-0.01, 4.0), (np.nan, 4.0), (np.inf, 4.0), (100.0, 1.0)):
        assert DO.lens(good, aperture, focus) is None
        assert call_lens(good, aperture, focus, start)[0] == -1, (aperture, focus)
    p = R.dof_params()
    assert hip_lib.rtHipDepthOfFieldLens(None, 0.01, 4.0, C.byref(p)) == -1 and "null" in R.last_error()
    assert hip_lib.rtHipDepthOfFieldLens(C.byref(R.Camera()), 0.01, 4.0, None) == -1 and "null" in R.last_error()
    got = R.dof_lens(good, 0.01, 4.0, rings=5)
    assert (got.focus, got.rings) == (F32(4.0), 5) and F32(got.cocScale).tobytes() == DO.lens(good, 0.01, 4.0)[1].tobytes()
    with pytest.raises(ValueError):
        R.dof_lens(DC.camera_dict(DC.LENS_DEGENERATE["parallel"]), 0.01, 4.0)


# ---- properties, on the oracle alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, W, H", [c for c in DC.CASES if c[1:] in ((33, 33), (64, 40))])
def test_no_aperture_or_everything_in_focus_returns_the_frame_bit_for_bit(name, W, H):
    colour, depth = DC.fields(name, W, H)
    for params in (DC.DEFAULT_LIKE, DC.ORDINARY[6]):
        assert DO.same_bits(DO.blur(colour, depth, **dict(params, coc_scale=0.0)), colour).all()
        flat = np.full_like(depth, params["focus"])
        assert DO.same_bits(DO.blur(colour, flat, **params), colour).all()
    if name not in ("focus", "constant"):  # (and with an aperture the field does blur)
        assert not DO.same_bits(DO.blur(colour, depth, **DC.DEFAULT_LIKE), colour).all()


def test_a_constant_colour_stays_within_a_few_ulp():
    value = np.asarray((0.3, 0.55, 0.8125), F32)
    worst, where = 0.0, None
    grid = DC.ORDINARY + tuple(p for p in DC.EXTREMES if p["coc_scale"] == 4096.0)
    for name, W, H in (c for c in DC.CASES if c[0] != "specials" and c[1:] in ((33, 33), (64, 40), DC.WIDE)):
        _, depth = DC.fields(name, W, H)
        colour = np.broadcast_to(value, (H, W, 3)).copy()
        for params in grid:
            out = DO.blur(colour, depth, **params)
            ulp = float((np.abs(out - colour) / np.spacing(colour)).max())
            if ulp > worst:
                worst, where = ulp, (name, W, H, params)
    print(f"a constant colour: at most {worst} ulp from the colour at {where} (measured {DC.CONSTANT_COLOUR_MEASURED_ULP}, "
          f"bound {DC.CONSTANT_COLOUR_ULP})")
    assert worst <= DC.CONSTANT_COLOUR_ULP  # measured 45 ulp, allowed 4 x 45 = 180 ulp (dof_cases.py)


def test_a_sharp_foreground_pixel_keeps_its_colour_bit_for_bit_beside_a_defocused_background():
    """depthSoftness = 0: a tap that lies behind p counts with min(rq, rp) = p's own half pixel, so where every ring tap lies a pixel or
    more from the centre -- R = maxCoc = 16 on 3 rings: the innermost at (1 - 0.375) / 3 * 16 = 3.3 pixels -- the sharp pixel's sum is
    its own centre tap, weight 1 / 0.25 = 4: a power of two, so colour * 4 / 4 is the colour."""
    name, W, H = "near_sharp", 64, 40
    colour, depth = DC.fields(name, W, H)
    sharp = depth == F32(DC.FOCUS)
    params = dict(focus=DC.FOCUS, coc_scale=24.0, max_coc=16.0, rings=3)
    parts = DO.blur(colour, depth, **params, depth_softness=0.0, with_parts=True)
    assert sharp.any() and (~sharp).any() and parts["gathered"].all() and (parts["r"][~sharp] == F32(16.0)).all()
    assert DO.same_bits(parts["out"][sharp], colour[sharp]).all()
    assert not DO.same_bits(parts["out"][~sharp], colour[~sharp]).all()  # while the background is blurred
    soft = DO.blur(colour, depth, **params, depth_softness=3e38)  # and with no depth test the background bleeds over the object
    assert not DO.same_bits(soft[sharp], colour[sharp]).all()


def test_the_defocused_backgrounds_blur_is_bounded_by_max_coc():
    W, H, edge = 128, 12, 64
    colour = np.empty((H, W, 3), F32)
    colour[:, :edge], colour[:, edge:] = F32(1.0), F32(0.25)  # (powers of two: a sum of c * w over equal c is c * wsum exactly)
    depth = np.full((H, W), 40.0, F32)
    x = np.arange(W)
    for max_coc, rings in ((5.0, 3), (16.0, 6), (1.0, 1)):
        out = DO.blur(colour, depth, focus=DC.FOCUS, coc_scale=4096.0, max_coc=max_coc, rings=rings)
        # a tap counts only below reff + 0.5 <= maxCoc + 0.5 from the centre, and lands at most sqrt(0.5) from its pixel's centre
        outside = np.abs(x + 0.5 - edge) > max_coc + 0.5 + 0.75
        assert (out[:, outside & (x < edge)] == F32(1.0)).all() and (out[:, outside & (x >= edge)] == F32(0.25)).all(), max_coc
        band = out[:, ~outside]
        assert ((band < 1.0) & (band > 0.25)).any(), max_coc  # and it is a ramp, not the step


def test_the_isolated_pixels_footprint_lies_inside_its_disc():
    name, W, H = "bright", 64, 40
    colour, depth = DC.fields(name, W, H)
    y, x = np.indices((H, W))
    dist = np.hypot(x - W // 2, y - H // 2)
    for coc_scale, rings in ((8.0, 3), (8.0, 6), (24.0, 4)):
        parts = DO.blur(colour, depth, focus=DC.FOCUS, coc_scale=coc_scale, max_coc=16.0, rings=rings, with_parts=True)
        r = float(parts["r"][H // 2, W // 2])
        assert r == min(coc_scale / 2, 16.0)  # depth 2 focus: a = 1/2
        lit = parts["out"].max(-1) > 0
        assert lit.sum() > 8 and dist[lit].max() <= r + 0.5 + 0.75, (coc_scale, rings, dist[lit].max())
        # the octagon: every ring of taps within the disc lights pixels in all eight directions
        assert lit[:H // 2].any() and lit[H // 2 + 1:].any() and lit[:, :W // 2].any() and lit[:, W // 2 + 1:].any()
        assert lit[(x - W // 2) * (y - H // 2) > 0].any() and lit[(x - W // 2) * (y - H // 2) < 0].any()


# ---- the GPU tests' inputs are not vacuous ------------------------------------------------------------------------------------------
def test_the_synthetic_fields_take_both_arms_and_skip_taps_at_the_border():
    parts = DO.blur(*DC.fields("split", *DC.WIDE), **DC.DEFAULT_LIKE, with_parts=True)
    copy, gather = DC.shares(parts)
    print(f"split {DC.WIDE}: copy {copy:.3f}, gather {gather:.3f}")
    assert np.allclose((copy, gather), DC.SPLIT_SHARES, atol=0.0015) and copy >= DC.MIN_COPY and gather >= DC.MIN_GATHER
    assert (parts["nb_max"] < 0.5).any() and (parts["nb_max"] >= 0.5).any()  # both arms in ONE launch
    full = DO.tap_count(DC.DEFAULT_LIKE["rings"]) - 1
    parts = DO.blur(*DC.fields("layers", 64, 40), **DC.DEFAULT_LIKE, with_parts=True)
    assert parts["gathered"].all() and (parts["taps"] < full).any() and (parts["taps"] == full).any()  # taps leave the image at its border
    assert DO.tap_count(3) == 49 and DO.tap_count(6) == 169 and len(DO.taps(6)) == 168
    for name in ("near_sharp", "near_blurred", "ramp", "misses", "layers"):
        r = DO.blur(*DC.fields(name, 64, 40), **DC.DEFAULT_LIKE, with_parts=True)["r"]
        assert (r < 0.5).any() and (r > 2.0).any(), name  # sharp and blurred pixels side by side
    # INTERIOR: three tile rows, so tiles with a neighbour above AND below and two with all eight; under `near_sharp` the disc in focus
    # lies inside the middle row, whose tiles take their radius from the 3 x 3 maximum
    for name in ("layers", "near_sharp"):
        parts = DO.blur(*DC.fields(name, *DC.INTERIOR), **DC.DEFAULT_LIKE, with_parts=True)
        assert parts["tile_max"].shape == (3, 4) and parts["gathered"].mean() >= DC.MIN_GATHER, name
        assert not DO.same_bits(parts["out"], DC.fields(name, *DC.INTERIOR)[0]).all(), name
    # TALL: 257 tiles in one column, the last past the first 256; along the ramp both arms are taken, the radius differs from tile to
    # tile, and the last tiles take their maximum from the neighbour below, across the boundary between tiles 255 and 256
    for name in ("ramp", "layers"):
        parts = DO.blur(*DC.fields(name, *DC.TALL), **DC.DEFAULT_LIKE, with_parts=True)
        assert parts["tile_max"].shape == (257, 1), name
        assert parts["gathered"][8192:].all() and parts["taps"][8192:].max() > 0, name  # tile 256 gathers
    ramp = DO.blur(*DC.fields("ramp", *DC.TALL), **DC.DEFAULT_LIKE, with_parts=True)
    copy, gather = DC.shares(ramp)
    print(f"ramp {DC.TALL}: copy {copy:.3f}, gather {gather:.3f}")
    assert copy > 0 and gather >= DC.MIN_GATHER
    assert not DO.same_bits(ramp["out"][8192:], DC.fields("ramp", *DC.TALL)[0][8192:]).all()  # (tile 256 is blurred: r = 6 there)
    assert ramp["nb_max"][255, 0] == ramp["tile_max"][256, 0] > ramp["tile_max"][255, 0] and len(np.unique(ramp["nb_max"])) > 100
    tiny = next(p for p in DC.EXTREMES if p["coc_scale"] == DC.DENORMAL and p["focus"] == 3e38 and p["max_coc"] == 32.0)
    r = DO.blur(*DC.fields("specials", 64, 40), **tiny, with_parts=True)["r"]  # cocScale the smallest denormal
    assert 0 < (r >= 0.5).sum() < 40 and set(np.unique(r[r >= 0.5])) == {F32(32.0)}  # only where a depth makes `a` infinite
