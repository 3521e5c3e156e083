"""Temporal accumulation without a GPU: the C ABI declares and exports the entry points and refuses NULL arguments and parameters out of
range; the numpy restatement (temporal_oracle.py) gives the known answers -- a still image converges on its count, a whole-pixel shift
copies the shifted history, maxHistory = 1 returns the frame, every kind of invalid history starts again, the background accumulates --;
and the inputs of tests/test_temporal_gpu.py (temporal_cases.py) are not vacuous.  The device is checked against the same restatement
there."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import motion_cases as MC
import temporal_cases as TC
import temporal_oracle as TO
from conftest import ROOT
from opencl_render_amd import raytrace as R

F32 = np.float32
NONE = 0xFFFFFFFF
ENTRY_POINTS = ("rtHipTemporalDevice", "rtHipTemporal", "rtHipSceneTemporal", "rtHipSceneTemporalReset", "rtHipSceneTemporalTimes")


def test_header_declares_the_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert re.search(r"\bvoid\s+rtHipTemporalDefaults\s*\(", text) and hasattr(hip_lib, "rtHipTemporalDefaults")
    assert "TEMPORAL ACCUMULATION" in text and text.index("MOTION VECTORS") < text.index("TEMPORAL ACCUMULATION")
    for method in ("temporal", "reset_temporal", "temporal_times_ms"):
        assert callable(getattr(R.ResidentScene, method))
    assert callable(R.temporal)
    p = R.TemporalParams()
    hip_lib.rtHipTemporalDefaults(C.byref(p))
    assert (p.maxHistory, p.depthTolerance) == (F32(32.0), F32(0.05))
    assert R.TEMPORAL_DEFAULTS == dict(max_history=32.0, depth_tolerance=0.05) == TO.DEFAULTS


def test_null_arguments_and_bad_parameters_are_refused_without_a_device():
    """(Nothing here reaches a device: the parameters and the NULL checks come first.)"""
    L = R.lib()
    W, H = 4, 3
    f = [np.full((H, W, 3), -3.0, F32) for _ in range(10)]
    ptr = [a.ctypes.data_as(C.c_void_p) for a in f]
    good = R.temporal_params()
    assert L.rtHipSceneTemporal(None, C.byref(good), None, ptr[0], None, None, None, None) == -1 and "null" in R.last_error()
    assert L.rtHipSceneTemporalReset(None) == -1 and "null" in R.last_error()
    assert L.rtHipSceneTemporalTimes(None, (C.c_float * 4)()) == -1 and "null" in R.last_error()
    for call, tail in ((L.rtHipTemporal, ()), (L.rtHipTemporalDevice, (None,))):
        assert call(0, W, H, *ptr, None, *tail) == -1 and "null parameters" in R.last_error()
        for i in range(9):  # every array but outCount is needed
            args = list(ptr)
            args[i] = None
            assert call(0, W, H, *args, C.byref(good), *tail) == -1 and "null array" in R.last_error(), i
        for bad in (dict(max_history=0.5), dict(max_history=65537.0), dict(max_history=np.nan), dict(max_history=np.inf),
                    dict(depth_tolerance=-0.01), dict(depth_tolerance=np.nan), dict(depth_tolerance=np.inf)):
            assert call(0, W, H, *ptr, C.byref(R.temporal_params(**bad)), *tail) == -1, bad
            assert ("maxHistory" if "max_history" in bad else "depthTolerance") in R.last_error()
        for w, h in ((0, 3), (4, 0), (16385, 1), (1, 16385)):
            assert call(0, w, h, *ptr, C.byref(good), *tail) == -1 and "image" in R.last_error(), (w, h)
    assert all((a == -3.0).all() for a in f)
    with pytest.raises(ValueError):
        R.temporal(f[0], f[1][..., :2].copy(), f[2][..., 0].copy(), np.zeros((H, W), np.uint32), dict(colour=f[0]))  # a history without its guides


# ---- known answers on the oracle alone ---------------------------------------------------------------------------------------------
def still(W=9, H=7, value=(0.25, 0.5, 0.8125)):
    """A still view of one surface: zero motion, prev_t = t, one triangle."""
    colour = np.broadcast_to(np.asarray(value, F32), (H, W, 3)).copy()
    return colour, np.zeros((H, W, 2), F32), np.full((H, W), 4.0, F32), np.full((H, W), 5, np.uint32)


def test_zero_motion_and_a_constant_colour_converge_on_the_count():
    colour, motion, t, tri = still()
    for cap in (32.0, 3.0, 1.0):
        hist = TO.empty_history(*t.shape)
        for n in range(1, 41):
            out = TO.accumulate(colour, motion, t, tri, hist, max_history=cap)
            assert (out["count"] == F32(min(n, cap))).all(), (cap, n)
            assert out["colour"].tobytes() == colour.tobytes(), (cap, n)  # hc + (c - hc) * a with c == hc: exact
            hist = TO.next_history(out, t, tri)


def test_a_whole_pixel_shift_copies_the_shifted_history_and_resets_what_comes_from_outside():
    W, H = 12, 8
    rng = np.random.default_rng(5)
    hist = dict(colour=rng.random((H, W, 3), dtype=F32), count=np.full((H, W), 1.0, F32), t=np.full((H, W), 4.0, F32),
                triangle=np.full((H, W), 5, np.uint32))
    colour = rng.random((H, W, 3), dtype=F32)
    motion = np.zeros((H, W, 2), F32)
    motion[..., 0] = 2.0  # the surface was two pixels to the right: ax = ay = 0, the weights are 1, 0, 0, 0
    # a frame that equals the shifted history: hc + (c - hc) * a with c == hc returns the history pixel exactly
    same = np.empty_like(colour)
    same[:, :W - 2] = hist["colour"][:, 2:]
    same[:, W - 2:] = colour[:, W - 2:]
    out = TO.accumulate(same, motion, np.full((H, W), 4.0, F32), np.full((H, W), 5, np.uint32), hist, with_taps=True)
    assert out["colour"][:, :W - 2].tobytes() == hist["colour"][:, 2:].tobytes()
    assert (out["count"][:, :W - 2] == 2.0).all() and (out["taps"][:, :W - 2] >= 1).all()
    # columns whose source lies outside the image start again: W - 2 has gx = W, outside the range; W - 1 likewise
    assert (out["count"][:, W - 2:] == 1.0).all() and not out["used"][:, W - 2:].any()
    assert out["colour"][:, W - 2:].tobytes() == same[:, W - 2:].tobytes()
    # and with another colour the blend is hc + (c - hc) / 2 of the SHIFTED history pixel
    out = TO.accumulate(colour, motion, np.full((H, W), 4.0, F32), np.full((H, W), 5, np.uint32), hist)
    hc = hist["colour"][:, 2:]
    assert out["colour"][:, :W - 2].tobytes() == (hc + (colour[:, :W - 2] - hc) * F32(0.5)).tobytes()


def test_max_history_one_returns_the_frame_bit_for_bit():
    for W, H in TC.SIZES[1:]:
        colour, motion, prev_t, tri, hist = TC.fields(W, H)
        # (an infinite history length times a weight of 0 is a NaN length, which no maxHistory bounds: those lengths are made finite here)
        hist = dict(hist, count=np.where(np.isfinite(hist["count"]), hist["count"], F32(2.0)))
        out = TO.accumulate(colour, motion, prev_t, tri, hist, max_history=1.0, with_taps=True)
        assert out["used"].mean() > 0.5 and np.isnan(hist["colour"]).any()
        assert TO.same_bits(out["colour"], colour).all() and (out["count"] == 1.0).all()
        blended = TO.accumulate(colour, motion, prev_t, tri, hist, max_history=2.0)
        assert not TO.same_bits(blended["colour"], colour).all()


def test_every_kind_of_invalid_history_starts_again():
    colour, motion, t, tri = still()
    H, W = t.shape
    good = dict(colour=np.full((H, W, 3), 0.5, F32), count=np.full((H, W), 4.0, F32), t=t.copy(), triangle=tri.copy())
    base = TO.accumulate(colour, motion, t, tri, good)
    assert (base["count"] == 5.0).all()
    cases = {
        "triangle mismatch": dict(history=dict(good, triangle=tri + np.uint32(1))),
        "prev_t zero": dict(prev_t=np.zeros_like(t)),
        "prev_t negative": dict(prev_t=-t),
        "prev_t NaN": dict(prev_t=np.full_like(t, np.nan)),
        "NaN motion": dict(motion=np.full_like(motion, np.nan)),
        "infinite motion": dict(motion=np.full_like(motion, np.inf)),
        "no history": dict(history=dict(good, count=np.zeros_like(t))),
        "history shorter than a frame": dict(history=dict(good, count=np.full_like(t, 0.99))),
        "NaN history count": dict(history=dict(good, count=np.full_like(t, np.nan))),
        "depth beyond the tolerance": dict(history=dict(good, t=t * F32(1.06))),
    }
    for name, change in cases.items():
        args = dict(colour=colour, motion=motion, prev_t=t, triangle=tri, history=good)
        args.update(change)
        out = TO.accumulate(**args)
        assert (out["count"] == 1.0).all() and out["colour"].tobytes() == colour.tobytes(), name
    inside = TO.accumulate(colour, motion, t, tri, dict(good, t=t * F32(1.04)))  # within 5 %
    assert (inside["count"] == 5.0).all()


def test_a_missed_pixel_over_missed_history_accumulates():
    colour, motion, t, tri = still()
    inf, none = np.full_like(t, np.inf), np.full_like(tri, NONE)
    hist = dict(colour=np.full(colour.shape, 0.5, F32), count=np.full_like(t, 2.0), t=inf, triangle=none)
    out = TO.accumulate(colour, motion, inf, none, hist)  # inf - inf is NaN: only the == arm accepts
    assert (out["count"] == 3.0).all()
    over_geometry = TO.accumulate(colour, motion, inf, none, dict(hist, t=t, triangle=tri))
    assert (over_geometry["count"] == 1.0).all()


# ---- the kernel's per-pixel code, compiled for the host ---------------------------------------------------------------------------------
HOST_FLAGS = ["-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]  # csrc/Makefile's exactness flags


@pytest.fixture(scope="module")
def host_pixel(tmp_path_factory):
    """tests/temporal_host.cpp (csrc/rt_temporal_pixel.h, what rtt_accumulate_kernel runs per lane) as a host library."""
    import subprocess
    out = tmp_path_factory.mktemp("temporal_host") / "libtemporal_host.so"
    subprocess.run([os.environ.get("CXX", "g++")] + HOST_FLAGS + ["-I", os.path.join(ROOT, "opencl_render_amd", "csrc"), "-o", str(out),
                    os.path.join(ROOT, "tests", "temporal_host.cpp")], check=True)
    lib = C.CDLL(str(out))
    lib.temporal_host.restype = None
    lib.temporal_host.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 10 + [C.c_float, C.c_float]

    def run(colour, motion, prev_t, triangle, history, max_history=TO.DEFAULTS["max_history"], depth_tolerance=TO.DEFAULTS["depth_tolerance"]):
        H, W = prev_t.shape
        ins = [np.ascontiguousarray(a) for a in (colour, motion, prev_t, triangle, history["colour"], history["count"], history["t"],
                                                 history["triangle"])]
        out = dict(colour=np.full((H, W, 3), -7.0, F32), count=np.full((H, W), -7.0, F32))
        lib.temporal_host(W, H, *[a.ctypes.data for a in ins], out["colour"].ctypes.data, out["count"].ctypes.data, max_history, depth_tolerance)
        return out

    return run


@pytest.mark.parametrize("W, H", TC.SIZES)
def test_the_kernels_pixel_code_on_the_host_equals_the_oracle_bit_for_bit(host_pixel, W, H):
    fields = TC.fields(W, H)
    for params in ({}, dict(max_history=4.0, depth_tolerance=0.0), dict(max_history=1.0), dict(max_history=65536.0, depth_tolerance=0.3)):
        want, got = TO.accumulate(*fields, **params), host_pixel(*fields, **params)
        for k in ("colour", "count"):
            bad = np.flatnonzero(~TO.same_bits(got[k], want[k]).reshape(-1))
            assert bad.size == 0, f"{W}x{H} {params}: {k} differs in {bad.size} values, first {bad[:4]}"


def test_the_kernels_pixel_code_on_the_host_gives_the_known_answers(host_pixel):
    colour, motion, t, tri = still()
    for cap in (32.0, 3.0, 1.0):
        hist = TO.empty_history(*t.shape)
        for n in range(1, 41):
            out = host_pixel(colour, motion, t, tri, hist, max_history=cap)
            assert (out["count"] == F32(min(n, cap))).all() and out["colour"].tobytes() == colour.tobytes(), (cap, n)
            hist = TO.next_history(out, t, tri)
    inf, none = np.full_like(t, np.inf), np.full_like(tri, NONE)
    sky = dict(colour=np.full(colour.shape, 0.5, F32), count=np.full_like(t, 2.0), t=inf, triangle=none)
    assert (host_pixel(colour, motion, inf, none, sky)["count"] == 3.0).all()
    assert (host_pixel(colour, motion, inf, none, dict(sky, t=t, triangle=tri))["count"] == 1.0).all()


# ---- the GPU tests' inputs are not vacuous ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", TC.SIZES[1:])
def test_the_synthetic_fields_take_every_path(W, H):
    out = TO.accumulate(*TC.fields(W, H), with_taps=True)
    full, some, reset = TC.shares(out)
    print(f"{W} x {H}: all four taps {full:.3f}, some {some:.3f}, reset {reset:.3f}")
    assert full >= TC.MIN_ALL_TAPS and some >= TC.MIN_SOME_TAPS and reset >= TC.MIN_RESET
    assert np.isnan(out["colour"]).any() and (out["count"] == 32.0).any() and (out["inside"][out["used"]] < 4).any()


@pytest.mark.parametrize("name", list(TC.CAMERA_SCENES))
def test_camera_chains_are_not_vacuous(name):
    sc = MC.base_scene(name, TC.CAMERA_SCENES[name])
    accept, refused = TC.chain_shares(TC.chain_flows([(cur, ref) for _, cur, ref in TC.camera_chain(sc)]))
    print(f"{name}: {accept:.3f} of the hit pixels accept history in some step, {refused} pixels are refused a tap")
    assert accept >= TC.MIN_ACCEPT and refused >= 1


def test_the_geometry_chain_is_not_vacuous():
    sc = MC.base_scene(TC.GEOMETRY_SCENE, MC.GEOMETRY_SCENES[TC.GEOMETRY_SCENE])
    accept, refused = TC.chain_shares(TC.chain_flows([(cur, ref) for _, _, cur, ref in TC.geometry_chain(sc)]))
    print(f"{TC.GEOMETRY_SCENE}: {accept:.3f} of the hit pixels accept history in some step, {refused} pixels are refused a tap")
    assert accept >= TC.MIN_ACCEPT and refused >= 1
