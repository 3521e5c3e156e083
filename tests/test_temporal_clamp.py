"""The temporal clamp without a GPU: the C ABI declares and exports the entry points and refuses bad parameters before anything needs a
device; the kernel's per-pixel code, compiled for the host, equals the numpy restatement (temporal_clamp_oracle.py) bit for bit on
perturbed and on special-valued fields; the restatement gives the known answers and reduces to the unclamped oracles where nothing is
moved; and the inputs of tests/test_temporal_clamp_gpu.py (temporal_clamp_cases.py) are not vacuous.  The device is checked against the
same restatement there."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_clamp_cases as CC
import temporal_clamp_oracle as CO
import temporal_oracle as TO
import variance_oracle as VO
from conftest import ROOT
from test_temporal import HOST_FLAGS
from opencl_render_amd import raytrace as R

F32 = np.float32
ENTRY_POINTS = ("rtHipTemporalClampCheck", "rtHipTemporalClampDevice", "rtHipTemporalClamp", "rtHipTemporalMomentsClampDevice",
                "rtHipTemporalMomentsClamp", "rtHipSceneSetTemporalClamp", "rtHipSceneGetTemporalClamp")


def test_header_declares_the_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert re.search(r"\bvoid\s+rtHipTemporalClampDefaults\s*\(", text) and hasattr(hip_lib, "rtHipTemporalClampDefaults")
    assert text.index("VARIANCE-GUIDED FILTER:") < text.index("TEMPORAL CLAMP:") < text.index("AMBIENT OCCLUSION BAKE:")
    assert re.search(r"#define\s+RT_HIP_CLAMP_MINMAX\s+1u", text) and re.search(r"#define\s+RT_HIP_CLAMP_VARIANCE\s+2u", text)
    for method in ("set_temporal_clamp", "temporal_clamp"):
        assert callable(getattr(R.ResidentScene, method))
    p = R.TemporalClampParams()
    hip_lib.rtHipTemporalClampDefaults(C.byref(p))
    assert (p.mode, p.gamma) == (3, 1.0)
    assert R.TEMPORAL_CLAMP_DEFAULTS == dict(mode=3, gamma=1.0) == CO.DEFAULTS
    assert R.TEMPORAL_CLAMP_MODES == dict(minmax=CO.MINMAX, variance=CO.VARIANCE, both=CO.BOTH)


BAD_CLAMPS = (dict(mode=0), dict(mode=4), dict(mode=0xFFFFFFFF), dict(gamma=np.nan), dict(gamma=-0.5), dict(gamma=np.inf),
              dict(gamma=-np.inf))


def test_bad_parameters_and_a_null_clamp_are_refused_without_a_device():
    """(Nothing here reaches a device: the parameter checks come first.)"""
    L = R.lib()
    assert L.rtHipTemporalClampCheck(None) == -1 and "null" in R.last_error()
    for bad in BAD_CLAMPS:
        assert L.rtHipTemporalClampCheck(C.byref(R.temporal_clamp_params(**bad))) == -1, bad
        assert ("mode" if "mode" in bad else "gamma") in R.last_error()
    for mode in CC.MODES:
        for gamma in (0.0, 1.0, 2.5, 3e38):
            assert L.rtHipTemporalClampCheck(C.byref(R.temporal_clamp_params(mode, gamma))) == 0, (mode, gamma)
    assert L.rtHipSceneSetTemporalClamp(None, C.byref(R.temporal_clamp_params())) == -1 and "null" in R.last_error()
    assert L.rtHipSceneGetTemporalClamp(None, C.byref(R.TemporalClampParams())) == -1 and "null" in R.last_error()
    W, H = 4, 3
    f = [np.full((H, W, 3), -3.0, F32) for _ in range(13)]
    ptr = [a.ctypes.data_as(C.c_void_p) for a in f]
    good = R.temporal_params()
    calls = ((L.rtHipTemporalClamp, 10, ()), (L.rtHipTemporalClampDevice, 10, (None,)), (L.rtHipTemporalMomentsClamp, 13, ()),
             (L.rtHipTemporalMomentsClampDevice, 13, (None,)))
    for call, n, tail in calls:
        assert call(0, W, H, *ptr[:n], C.byref(good), None, *tail) == -1 and "null parameters" in R.last_error()
        for bad in BAD_CLAMPS:
            assert call(0, W, H, *ptr[:n], C.byref(good), C.byref(R.temporal_clamp_params(**bad)), *tail) == -1, bad
            assert "temporal clamp" in R.last_error()
        clamp = R.temporal_clamp_params()
        assert call(0, W, H, *ptr[:n], None, C.byref(clamp), *tail) == -1 and "null parameters" in R.last_error()
        assert call(0, W, H, *ptr[:n], C.byref(R.temporal_params(max_history=0.5)), C.byref(clamp), *tail) == -1 and "maxHistory" in R.last_error()
        assert call(0, 0, H, *ptr[:n], C.byref(good), C.byref(clamp), *tail) == -1 and "image" in R.last_error()
        args = list(ptr[:n])
        args[0] = None
        assert call(0, W, H, *args, C.byref(good), C.byref(clamp), *tail) == -1 and "null array" in R.last_error()
    assert all((a == -3.0).all() for a in f)
    with pytest.raises(ValueError):
        R.temporal_clamp_params(mode="sharp")
    with pytest.raises(TypeError):
        R.temporal(f[0], f[1][..., :2].copy(), f[2][..., 0].copy(), np.zeros((H, W), np.uint32), TO.empty_history(H, W), clamp=dict(sigma=1.0))


# ---- the kernel's per-pixel code, compiled for the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_pixel(tmp_path_factory):
    """tests/temporal_clamp_host.cpp (csrc/rt_temporal_clamp_pixel.h, what rtt_clamp_kernel runs per lane) as a host library."""
    out = tmp_path_factory.mktemp("temporal_clamp_host") / "libtemporal_clamp_host.so"
    subprocess.run([os.environ.get("CXX", "g++")] + HOST_FLAGS + ["-I", os.path.join(ROOT, "opencl_render_amd", "csrc"), "-o", str(out),
                    os.path.join(ROOT, "tests", "temporal_clamp_host.cpp")], check=True)
    lib = C.CDLL(str(out))
    lib.temporal_clamp_host.restype = None
    lib.temporal_clamp_host.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 13 + [C.c_float, C.c_float, C.c_uint32, C.c_float]

    def run(colour, motion, prev_t, triangle, history, max_history=TO.DEFAULTS["max_history"], depth_tolerance=TO.DEFAULTS["depth_tolerance"],
            mode=CO.DEFAULTS["mode"], gamma=CO.DEFAULTS["gamma"]):
        H, W = prev_t.shape
        ins = [np.ascontiguousarray(a) for a in (colour, motion, prev_t, triangle, history["colour"], history["count"], history["t"],
                                                 history["triangle"])]
        out = dict(colour=np.full((H, W, 3), -7.0, F32), count=np.full((H, W), -7.0, F32))
        moments = np.ascontiguousarray(history["moments"]) if "moments" in history else None
        if moments is not None:
            out.update(moments=np.full((H, W, 2), -7.0, F32), variance=np.full((H, W), -7.0, F32))
        lib.temporal_clamp_host(W, H, *[a.ctypes.data for a in ins], moments.ctypes.data if moments is not None else None,
                                out["colour"].ctypes.data, out["count"].ctypes.data, *([out["moments"].ctypes.data, out["variance"].ctypes.data]
                                                                                       if moments is not None else [None, None]),
                                max_history, depth_tolerance, mode, gamma)
        return out

    return run


def assert_same(got, want, label):
    for k in got:
        bad = np.flatnonzero(~TO.same_bits(got[k], want[k]).reshape(-1))
        assert bad.size == 0, (f"{label}: {k} differs in {bad.size} values, first {bad[:4]}: got {got[k].reshape(-1)[bad[:4]]}, "
                               f"want {want[k].reshape(-1)[bad[:4]]}")


@pytest.mark.parametrize("W, H", CC.SHAPES)
def test_the_kernels_pixel_code_on_the_host_equals_the_oracle_bit_for_bit(host_pixel, W, H):
    for moments in (False, True):
        f = CC.fields(W, H, moments=moments)
        for mode in CC.MODES:
            for gamma in CC.GAMMAS:
                assert_same(host_pixel(*f, mode=mode, gamma=gamma), CO.accumulate(*f, mode=mode, gamma=gamma),
                            f"{W}x{H} mode {mode} gamma {gamma} moments {moments}")
        for params in (dict(max_history=4.0, depth_tolerance=0.0), dict(max_history=1.0), dict(max_history=65536.0, depth_tolerance=0.3)):
            assert_same(host_pixel(*f, **params), CO.accumulate(*f, **params), f"{W}x{H} {params} moments {moments}")


def test_special_values_in_frame_and_history_have_the_oracles_answer(host_pixel):
    """NaN, +-inf, subnormal, -0 and overflowing colours in frame and history."""
    W, H = CC.SPECIAL_SHAPE
    for moments in (False, True):
        f = CC.special_fields(W, H, moments=moments)
        for a in (f[0], f[4]["colour"]):
            assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any() and (np.abs(a) == F32(1e-40)).any()
        for mode in CC.MODES:
            for gamma in CC.GAMMAS:
                want = CO.accumulate(*f, mode=mode, gamma=gamma)
                assert_same(host_pixel(*f, mode=mode, gamma=gamma), want, f"special mode {mode} gamma {gamma} moments {moments}")
        assert np.isnan(want["colour"]).any() and np.isinf(want["colour"]).any()


# ---- known answers ------------------------------------------------------------------------------------------------------------------------
def constant_case(W=9, H=7, frame=(0.25, 0.5, 0.8125), old=(0.75, 0.125, 0.3125), count=4.0):
    """A constant frame over a constant, different, fully valid history of the same surface, zero motion.  The values have few
    mantissa bits, so that the box's sums and squares are exact and its mean is the value itself."""
    colour = np.broadcast_to(np.asarray(frame, F32), (H, W, 3)).copy()
    t, tri = np.full((H, W), 4.0, F32), np.full((H, W), 5, np.uint32)
    hist = dict(colour=np.broadcast_to(np.asarray(old, F32), (H, W, 3)).copy(), count=np.full((H, W), count, F32), t=t.copy(), triangle=tri.copy())
    return colour, np.zeros((H, W, 2), F32), t, tri, hist


def test_a_constant_frame_over_a_different_history_returns_the_frame(host_pixel):
    """The box of a constant frame is the point c, so the history is pulled onto c and c + (c - c) * a is c: in every mode, at every
    gamma, the output is the frame and the count is the unclamped call's.  Unclamped, the old colour drags on: this fails without the
    feature."""
    f = constant_case()
    plain = TO.accumulate(*f)
    assert (plain["count"] == 5.0).all() and not (plain["colour"] == f[0]).any()
    for mode in CC.MODES:
        for gamma in CC.GAMMAS:
            for out in (CO.accumulate(*f, mode=mode, gamma=gamma), host_pixel(*f, mode=mode, gamma=gamma)):
                assert out["colour"].tobytes() == f[0].tobytes(), (mode, gamma)
                assert out["count"].tobytes() == plain["count"].tobytes(), (mode, gamma)
    f = constant_case(W=1, H=1)
    assert CO.accumulate(*f)["colour"].tobytes() == f[0].tobytes() and host_pixel(*f)["colour"].tobytes() == f[0].tobytes()
    # with moments: the colour is the frame, the moments are the unclamped call's (the old luminance still in them)
    fm = f[:4] + (dict(f[4], moments=np.full((1, 1, 2), 0.5, F32)),)
    out, plain = host_pixel(*fm), VO.accumulate(*fm)
    assert out["colour"].tobytes() == f[0].tobytes() and out["moments"].tobytes() == plain["moments"].tobytes()
    assert out["variance"].tobytes() == plain["variance"].tobytes() and (plain["variance"] > 0).all()


def test_a_history_inside_the_box_is_untouched_and_one_outside_lands_on_its_edge():
    """One pixel pair by hand: a frame of two columns 0.25 | 0.75 (every 3x3 box is [0.25, 0.75] under min/max), history 0.5 (inside)
    and 2.0 (outside, above), count 1, so a = 1/2."""
    W, H = 4, 3
    colour = np.zeros((H, W, 3), F32)
    colour[:, :2], colour[:, 2:] = 0.25, 0.75
    t, tri = np.full((H, W), 4.0, F32), np.full((H, W), 5, np.uint32)
    hist = dict(colour=np.full((H, W, 3), 0.5, F32), count=np.ones((H, W), F32), t=t.copy(), triangle=tri.copy())
    hist["colour"][:, 2:] = 2.0
    out = CO.accumulate(colour, np.zeros((H, W, 2), F32), t, tri, hist, mode=CO.MINMAX)
    assert (out["moved"][:, 1] == 0).all() and (out["colour"][:, 1] == F32(0.375)).all()  # 0.5 + (0.25 - 0.5) / 2
    assert (out["moved"][:, 2] == F32(-1.25)).all() and (out["colour"][:, 2] == F32(0.75)).all()  # pulled to 0.75 = the frame
    assert (out["colour"][:, 0] == F32(0.25)).all()  # column 0 sees 0.25 only: the box is a point
    assert (out["count"] == 2.0).all()


# ---- the clamp is an insertion: where it moves nothing, nothing changes ---------------------------------------------------------------------
@pytest.mark.parametrize("W, H", CC.SHAPES)
def test_where_nothing_is_moved_the_output_is_the_unclamped_oracles(W, H):
    for moments in (False, True):
        for f in (CC.fields(W, H, moments=moments), CC.special_fields(W, H, moments=moments)):
            plain = (VO if moments else TO).accumulate(*f)
            for mode in CC.MODES:
                for gamma in CC.GAMMAS:
                    out = CO.accumulate(*f, mode=mode, gamma=gamma)
                    still = ~(out["moved"] != 0).any(-1)
                    assert TO.same_bits(out["colour"], plain["colour"])[still].all(), (mode, gamma, moments)
                    assert TO.same_bits(out["count"], plain["count"]).all(), (mode, gamma, moments)
                    if moments:
                        assert TO.same_bits(out["moments"], plain["moments"]).all() and TO.same_bits(out["variance"], plain["variance"]).all()
                    assert not out["moved"][~out["used"]].any()  # no blend, no clamp


# ---- the GPU tests' inputs are not vacuous ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", [s for s in CC.SHAPES if s[0] * s[1] >= CC.MIN_PIXELS])
def test_the_perturbed_fields_move_some_pixels_and_leave_others(W, H):
    f = CC.fields(W, H)
    for mode in CC.MODES:
        out = CO.accumulate(*f, mode=mode, gamma=1.0)
        moved, unmoved = CC.moved_shares(out)
        print(f"{W} x {H} mode {mode}: of {int(out['used'].sum())} pixels with valid history {moved:.3f} have a channel moved, {unmoved:.3f} none")
        assert out["used"].sum() >= 50 and moved >= CC.MIN_MOVED and unmoved >= CC.MIN_UNMOVED
        far = np.abs(out["moved"]).max(-1)
        assert (far > 1.0).any() and ((far > 0) & (far < 0.25)).any()  # pulled in from far outside, and from just outside
