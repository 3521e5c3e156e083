"""Motion blur without a GPU: the C ABI declares and exports the entry points and refuses NULL arguments and parameters out of range, at
their legal edges too; the kernel's per-pixel code (csrc/rt_motion_blur_pixel.h) compiled for the host equals the numpy restatement
(motion_blur_oracle.py) bit for bit over every case of motion_blur_cases.py; the restatement has the properties a blur must have -- no
motion or no exposure copies the frame, a constant colour stays, a step edge under a uniform flow becomes a bounded monotone ramp, a still
near object keeps its interior beside a fast background --; and the inputs of tests/test_motion_blur_gpu.py are not vacuous.  The device
is checked against the same restatement there."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_blur_cases as BC
import motion_blur_oracle as BO
import motion_cases as MC
import motion_oracle as MO
from conftest import ROOT
from opencl_render_amd import raytrace as R

F32 = np.float32
ENTRY_POINTS = ("rtHipMotionBlurCheck", "rtHipMotionBlurDevice", "rtHipMotionBlur", "rtHipSceneMotionBlur", "rtHipSceneMotionBlurTimes")


def test_header_declares_the_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert re.search(r"\bvoid\s+rtHipMotionBlurDefaults\s*\(", text) and hasattr(hip_lib, "rtHipMotionBlurDefaults")
    assert re.search(r"\buint64_t\s+rtHipMotionBlurScratchBytes\s*\(", text) and hasattr(hip_lib, "rtHipMotionBlurScratchBytes")
    assert text.index("TEMPORAL CLAMP:") < text.index("MOTION BLUR:") < text.index("AMBIENT OCCLUSION BAKE:")
    for method in ("motion_blur", "motion_blur_times_ms"):
        assert callable(getattr(R.ResidentScene, method))
    assert callable(R.motion_blur)
    assert C.sizeof(R.MotionBlurParams) == 16
    assert [f[0] for f in R.MotionBlurParams._fields_] == ["shutter", "maxBlur", "taps", "depthSoftness"]
    p = R.MotionBlurParams()
    hip_lib.rtHipMotionBlurDefaults(C.byref(p))
    assert (p.shutter, p.maxBlur, p.taps, p.depthSoftness) == (F32(0.5), F32(16.0), 15, F32(0.05))
    assert R.MOTION_BLUR_DEFAULTS == dict(shutter=0.5, max_blur=16.0, taps=15, depth_softness=0.05) == BO.DEFAULTS


def test_parameter_refusals_and_their_legal_edges(hip_lib):
    check = lambda **kw: hip_lib.rtHipMotionBlurCheck(C.byref(R.motion_blur_params(**kw)))  # noqa: E731
    assert hip_lib.rtHipMotionBlurCheck(None) == -1 and "null parameters" in R.last_error()
    assert check() == 0
    edges = (dict(shutter=0.0), dict(shutter=4.0), dict(max_blur=1.0), dict(max_blur=32.0), dict(taps=1), dict(taps=64),
             dict(depth_softness=0.0), dict(depth_softness=3e38), dict(shutter=-0.0), dict(shutter=1e-45))
    for good in edges:
        assert check(**good) == 0, good
    below, above = np.nextafter(F32(1.0), F32(0.0)), np.nextafter(F32(32.0), F32(64.0))
    refused = (("shutter", dict(shutter=-1e-45)), ("shutter", dict(shutter=np.nextafter(F32(4.0), F32(5.0)))), ("shutter", dict(shutter=np.nan)),
               ("shutter", dict(shutter=np.inf)), ("shutter", dict(shutter=-np.inf)),
               ("maxBlur", dict(max_blur=below)), ("maxBlur", dict(max_blur=above)), ("maxBlur", dict(max_blur=0.0)),
               ("maxBlur", dict(max_blur=np.nan)), ("maxBlur", dict(max_blur=np.inf)),
               ("taps", dict(taps=0)), ("taps", dict(taps=65)), ("taps", dict(taps=0xFFFFFFFF)),
               ("depthSoftness", dict(depth_softness=-1e-45)), ("depthSoftness", dict(depth_softness=np.nan)),
               ("depthSoftness", dict(depth_softness=np.inf)))
    for word, bad in refused:
        assert check(**bad) == -1 and word in R.last_error(), bad
    with pytest.raises(ValueError):
        R.motion_blur_params(taps=-1)


def test_null_arguments_bad_parameters_and_bad_sizes_are_refused_without_a_device(hip_lib):
    """(Nothing here reaches a device: the parameters, the sizes and the NULL checks come first.)"""
    L = hip_lib
    W, H = 4, 3
    f = [np.full((H, W, 3), -3.0, F32) for _ in range(5)]
    ptr = [a.ctypes.data_as(C.c_void_p) for a in f]
    good = R.motion_blur_params()
    assert L.rtHipSceneMotionBlur(None, C.byref(good), ptr[0], None, None, None) == -1 and "null" in R.last_error()
    assert L.rtHipSceneMotionBlurTimes(None, (C.c_float * 3)()) == -1 and "null" in R.last_error()
    assert L.rtHipMotionBlurScratchBytes(0, 3) == 0 and L.rtHipMotionBlurScratchBytes(16385, 1) == 0 and L.rtHipMotionBlurScratchBytes(16384, 16384) == 0
    assert L.rtHipMotionBlurScratchBytes(33, 33) == ((33 * 33 * 8 + 15) // 16) * 16 + 2 * 4 * 16
    calls = ((lambda a, p, w=W, h=H: L.rtHipMotionBlur(0, w, h, *a[:4], p), 4),
             (lambda a, p, w=W, h=H: L.rtHipMotionBlurDevice(0, w, h, *a[:5], 1 << 20, p, None), 5))
    for call, arrays in calls:
        assert call(ptr, None) == -1 and "null parameters" in R.last_error()
        for i in range(arrays):
            args = list(ptr)
            args[i] = None
            assert call(args, C.byref(good)) == -1 and "null array" in R.last_error(), i
        assert call(ptr, C.byref(R.motion_blur_params(taps=0))) == -1 and "taps" in R.last_error()
        for w, h in ((0, 3), (4, 0), (16385, 1), (1, 16385), (16384, 16384)):
            assert call(ptr, C.byref(good), w, h) == -1 and "image" in R.last_error(), (w, h)
    assert L.rtHipMotionBlurDevice(0, W, H, *ptr[:5], 16, C.byref(good), None) == -1 and "scratch" in R.last_error()
    assert all((a == -3.0).all() for a in f)
    with pytest.raises(ValueError):
        R.motion_blur(f[0], f[1], f[2][..., 0].copy())  # a motion array of three channels


# ---- the kernel's per-pixel code, compiled for the host ---------------------------------------------------------------------------------
HOST_FLAGS = ["-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]  # csrc/Makefile's exactness flags


@pytest.fixture(scope="module")
def host_blur(tmp_path_factory):
    """tests/motion_blur_host.cpp (csrc/rt_motion_blur_pixel.h, with a sequential (b) and (c)) as a host library."""
    out = tmp_path_factory.mktemp("motion_blur_host") / "libmotion_blur_host.so"
    subprocess.run([os.environ.get("CXX", "g++")] + HOST_FLAGS + ["-I", os.path.join(ROOT, "opencl_render_amd", "csrc"), "-o", str(out),
                    os.path.join(ROOT, "tests", "motion_blur_host.cpp")], check=True)
    lib = C.CDLL(str(out))
    lib.motion_blur_host.restype = None
    lib.motion_blur_host.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_float, C.c_float, C.c_uint32, C.c_float]

    def run(colour, motion, depth, shutter, max_blur, taps, depth_softness):
        H, W = depth.shape
        out = np.full((H, W, 3), -7.0, F32)
        lib.motion_blur_host(W, H, colour.ctypes.data, motion.ctypes.data, depth.ctypes.data, out.ctypes.data, shutter, max_blur, taps,
                             depth_softness)
        return out

    return run


@pytest.mark.parametrize("name, W, H", BC.CASES)
def test_the_kernels_pixel_code_on_the_host_equals_the_oracle_bit_for_bit(host_blur, name, W, H):
    fields = BC.fields(name, W, H)
    for params in BC.grid_of(W, H):
        want, got = BC.reference(name, W, H, params), host_blur(*fields, **params)
        bad = np.flatnonzero(~BO.same_bits(got, want).reshape(-1))
        assert bad.size == 0, f"{name} {W}x{H} {params}: differs in {bad.size} values, first {bad[:4]}"


# ---- properties, on the oracle alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, W, H", [c for c in BC.CASES if c[1:] in ((65, 34), (97, 70))])
def test_zero_motion_or_a_closed_shutter_returns_the_frame_bit_for_bit(name, W, H):
    colour, motion, depth = BC.fields(name, W, H)
    for params in (dict(), dict(taps=64, max_blur=32.0, depth_softness=0.0)):
        assert BO.same_bits(BO.blur(colour, motion, depth, **dict(params, shutter=0.0)), colour).all()
        assert BO.same_bits(BO.blur(colour, np.zeros_like(motion), depth, **dict(params, shutter=4.0)), colour).all()
    if name != "specials":  # (and with an open shutter the field does blur)
        assert not BO.same_bits(BO.blur(colour, motion, depth), colour).all()


def test_a_constant_colour_stays_within_a_few_ulp():
    value = np.asarray((0.3, 0.55, 0.8125), F32)
    worst = 0.0
    for name, W, H in (c for c in BC.CASES if c[0] != "specials" and c[1:] in ((33, 33), (97, 70), BC.WIDE)):
        _, motion, depth = BC.fields(name, W, H)
        colour = np.broadcast_to(value, (H, W, 3)).copy()
        for params in BC.GRID[::5]:
            out = BO.blur(colour, motion, depth, **params)
            worst = max(worst, float((np.abs(out - colour) / np.spacing(colour)).max()))
    print(f"a constant colour: at most {worst} ulp from the colour (bound {BC.CONSTANT_COLOUR_ULP})")
    assert worst <= BC.CONSTANT_COLOUR_ULP


def test_a_step_edge_under_a_uniform_flow_becomes_a_bounded_monotone_ramp():
    W, H, edge = 128, 12, 64
    colour = np.empty((H, W, 3), F32)
    colour[:, :edge], colour[:, edge:] = F32(1.0), F32(0.25)  # (powers of two: a sum of c * w over equal c is c * wsum exactly)
    motion = np.zeros((H, W, 2), F32)
    motion[..., 0] = 12.0  # shutter 1: a half-extent of 6 pixels
    out = BO.blur(colour, motion, np.full((H, W), 3.0, F32), shutter=1.0, max_blur=32.0)
    x = np.arange(W)
    outside = np.abs(x + 0.5 - edge) > 6 + 1
    assert (out[:, outside & (x < edge)] == F32(1.0)).all() and (out[:, outside & (x >= edge)] == F32(0.25)).all()
    assert (np.diff(out, axis=1) <= 0).all()  # non-increasing across the edge, in every row and channel
    band = out[:, ~outside]
    assert ((band < 1.0) & (band > 0.25)).any() and (out[:, edge - 1] > out[:, edge]).all()  # and it is a ramp, not the step


def test_a_still_near_object_keeps_its_interior_beside_a_fast_far_background():
    W, H, x0, x1, half = 128, 40, 40, 88, 5  # the object covers columns x0..x1-1; motion (20, 0) at shutter 0.5: half-extent 5
    rng = np.random.default_rng(3)
    colour = rng.random((H, W, 3), dtype=F32)
    x = np.arange(W)
    near = (x >= x0) & (x < x1)
    motion = np.zeros((H, W, 2), F32)
    motion[:, ~near, 0] = 20.0
    depth = np.where(near, F32(1.0), F32(10.0))[None, :].repeat(H, 0)
    parts = BO.blur(colour, motion, depth, shutter=0.5, max_blur=16.0, depth_softness=0.05, with_parts=True)
    assert parts["gathered"][:, near].all()  # the object's tiles neighbour the background's: its pixels do gather
    interior = (x >= x0 + half + 1) & (x < x1 - half - 1)
    worst = float(np.abs(parts["out"][:, interior] - colour[:, interior]).max())
    print(f"still near object: interior pixels at most {worst} from their own colour (bound {BC.STILL_INTERIOR_BOUND})")
    assert worst <= BC.STILL_INTERIOR_BOUND
    edge = (x >= x0 - half) & (x < x0)  # while the background beside it is smeared
    assert float(np.abs(parts["out"][:, edge] - colour[:, edge]).max()) > 0.05


# ---- the GPU tests' inputs are not vacuous ------------------------------------------------------------------------------------------
def test_the_synthetic_fields_take_both_arms_and_the_cap():
    best = {}
    for name, W, H in (c for c in BC.CASES if c[0] in ("split", "random")):
        for shutter in BC.SHUTTERS:
            copy, gather, clamped = BC.shares(BO.blur(*BC.fields(name, W, H), shutter=shutter, max_blur=7.5, with_parts=True))
            b = best.setdefault(name, [0.0, 0.0, 0.0])
            best[name] = [max(b[0], copy), max(b[1], gather), max(b[2], clamped)]
            if (name, W, H) in BC.MEASURED and shutter == 0.5:
                print(f"{name} {W} x {H}: copy {copy:.3f}, gather {gather:.3f}, clamped {clamped:.3f}")
                assert np.allclose((copy, gather, clamped), BC.MEASURED[name, W, H], atol=0.0015)
    for name in ("split", "random"):
        assert best[name][0] >= BC.MIN_COPY and best[name][1] >= BC.MIN_GATHER, (name, best[name])
    assert best["random"][2] >= BC.MIN_CLAMPED
    copy, gather, _ = BC.MEASURED[("split",) + BC.WIDE]  # both arms in ONE image
    assert copy >= BC.MIN_COPY and gather >= BC.MIN_GATHER
    parts = BO.blur(*BC.fields("uniform", 97, 70), with_parts=True)
    assert parts["gathered"].all() and (parts["taps"] < 15).any() and (parts["taps"] == 15).any()  # taps leave the image at its border
    parts = BO.blur(*BC.fields("random", 97, 70), shutter=4.0, max_blur=7.5, with_parts=True)
    assert (parts["l"] == F32(7.5)).mean() > 0.9  # ties among capped pixels: l == maxBlur exactly


def test_the_tall_shape_reaches_the_tiles_past_the_first_256():
    """1 x 257 tiles.  Every setting of TALL_GRID is one of GRID and every tap count occurs once; under each open shutter the last tile
    (rows 8192..8199) gathers, sums taps that stay inside the two columns and changes its pixels; under `random` the tiles' dominant
    velocities differ, so (c) has to pick among three tiles, also across the boundary between tiles 255 and 256."""
    assert all(p in BC.GRID for p in BC.TALL_GRID) and sorted(p["taps"] for p in BC.TALL_GRID) == sorted(BC.TAPS)
    assert all(BC.grid_of(W, H) is (BC.TALL_GRID if (W, H) == BC.TALL else BC.GRID) for _, W, H in BC.CASES)
    assert {n for n, W, H in BC.CASES if (W, H) == BC.TALL} == {"random", "ties"}
    for name in ("random", "ties"):
        colour = BC.fields(name, *BC.TALL)[0]
        for params in BC.TALL_GRID:
            parts = BO.blur(*BC.fields(name, *BC.TALL), **params, with_parts=True)
            assert parts["tile_max"].shape == (257, 1, 3)
            last = parts["taps"][8192:]
            print(f"{name} {BC.TALL} {params}: gather share {parts['gathered'].mean():.3f}, taps summed per pixel of the last tile "
                  f"{last.min()}..{last.max()}")
            assert parts["gathered"][8192:].all() and last.max() > 0, (name, params)
            assert not BO.same_bits(parts["out"][8192:], colour[8192:]).all(), (name, params)
    parts = BO.blur(*BC.fields("random", *BC.TALL), **BC.TALL_GRID[2], with_parts=True)
    tm, nb = parts["tile_max"][:, 0], parts["nb_max"][:, 0]
    assert len(np.unique(tm[:, 2])) > 100 and abs(tm[:, 1]).min() > 20 * abs(tm[:, 0]).max()  # different lengths, all of them vertical
    took = [int(np.flatnonzero((tm[max(t - 1, 0):t + 2] == nb[t]).all(-1))[0]) + max(t - 1, 0) - t for t in range(257)]
    assert {-1, 0, 1} == set(took) and (took[255] == 1 or took[256] == -1), "no tile takes its velocity across tiles 255 | 256"
    assert (parts["taps"] == 15).mean() > 0.5  # (vertical: most taps stay inside the image)


def test_ties_are_won_by_the_first_index():
    W, H = 97, 70
    _, motion, _ = BC.fields("ties", W, H)
    parts = BO.blur(*BC.fields("ties", W, H), with_parts=True)
    assert np.unique(parts["l"]).size == 1
    first = motion[::32, ::32] * F32(0.25)  # the velocity of each tile's first pixel at shutter 0.5
    assert parts["tile_max"][..., :2].tobytes() == np.ascontiguousarray(first).tobytes()
    # and the order matters: in some tile the last pixel points elsewhere, and the tiles do not all agree
    last = np.stack([[motion[min(ty * 32 + 31, H - 1), min(tx * 32 + 31, W - 1)] for tx in range(4)] for ty in range(3)]) * F32(0.25)
    assert (last != first).any() and np.unique(first.reshape(-1, 2), axis=0).shape[0] > 1
    nb = parts["nb_max"]  # (c): the first of the neighbourhood in its own order, which is the top-left neighbour that exists
    assert nb[1, 1].tobytes() == parts["tile_max"][0, 0].tobytes() and nb[0, 0].tobytes() == parts["tile_max"][0, 0].tobytes()
    assert nb[2, 3].tobytes() == parts["tile_max"][1, 2].tobytes()


def scene_shares(cur, ref, params):
    flow = MO.motion(cur, ref)
    colour = np.zeros((cur.height, cur.width, 3), F32)
    return float(BO.blur(colour, flow["motion"], flow["t"], **params, with_parts=True)["gathered"].mean())


@pytest.mark.parametrize("name", list(BC.CAMERA_SCENES))
def test_camera_scenes_are_not_vacuous(name):
    sc = MC.base_scene(name, BC.CAMERA_SCENES[name])
    got = {pose: round(scene_shares(cur, ref, BC.SCENE_PARAMS[0]), 3) for pose, cur, ref, _, _ in MC.camera_steps(sc)}
    print(f"{name}: gather shares per step {got}")
    assert got == BC.SCENE_GATHER_SHARES["camera", name] and max(got.values()) >= BC.MIN_GATHER


def test_the_geometry_scene_is_not_vacuous():
    name = BC.GEOMETRY_SCENE
    sc = MC.base_scene(name, MC.GEOMETRY_SCENES[name])
    got = {change: round(scene_shares(cur, ref, BC.SCENE_PARAMS[0]), 3) for change, _, cur, ref, _, _ in MC.geometry_steps(sc)}
    print(f"{name}: gather shares per step {got}")
    assert got == BC.SCENE_GATHER_SHARES["geometry", name] and max(got.values()) >= BC.MIN_GATHER
