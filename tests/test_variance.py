"""The variance-guided filter without a GPU: the C ABI declares and exports the entry points and refuses NULL arguments and parameters out
of range before any device is touched; the kernels' per-pixel code (csrc/rt_variance_pixel.h) compiled for the host equals the numpy
restatement (variance_oracle.py) bit for bit in all three stages; the restatement gives the known answers -- the colour and count of
TEMPORAL ACCUMULATION, the DENOISER without its colour edge-stop under an infinite variance, 4900/65536 of a unit variance after one
iteration on a flat image, variance 0 for constant frames --; and the inputs of tests/test_variance_gpu.py (variance_cases.py) are not
vacuous.  The device is checked against the same restatement there."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_oracle as DO
import temporal_cases as TC
import temporal_oracle as TO
import variance_cases as VC
import variance_oracle as VO
from conftest import ROOT
from test_temporal import HOST_FLAGS, still
from opencl_render_amd import raytrace as R

F32 = np.float32
ENTRY_POINTS = ("rtHipTemporalMomentsDevice", "rtHipTemporalMoments", "rtHipDenoiseVarianceDevice", "rtHipDenoiseVariance",
                "rtHipSceneTemporalVariance")
# parameter sets of the filter: the defaults; no spatial arm, a short filter; every pixel spatial, other weights; K = 0
FILTER_PARAMS = ({}, dict(spatial_below=0.0, iterations=2, luminance_sigma2=0.0), dict(spatial_below=65537.0, iterations=3, luminance_sigma2=0.5,
                 variance_floor=2.0 ** -100, albedo_inv_sigma2=3.0, normal_power_log2=2), dict(iterations=0))


def test_header_declares_the_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert re.search(r"\bvoid\s+rtHipVarianceDefaults\s*\(", text) and hasattr(hip_lib, "rtHipVarianceDefaults")
    assert re.search(r"\buint64_t\s+rtHipVarianceScratchBytes\s*\(", text) and hasattr(hip_lib, "rtHipVarianceScratchBytes")
    assert text.index("TEMPORAL ACCUMULATION") < text.index("VARIANCE-GUIDED FILTER")
    assert callable(R.ResidentScene.temporal_variance) and callable(R.temporal_moments) and callable(R.denoise_variance)
    p = R.VarianceParams()
    hip_lib.rtHipVarianceDefaults(C.byref(p))
    got = (p.iterations, p.luminanceSigma2, p.varianceFloor, p.albedoInvSigma2, p.normalPowerLog2, p.spatialBelow)
    assert got == (4, F32(R.VARIANCE_DEFAULTS["luminance_sigma2"]), F32(1e-8), F32(100.0), 7, F32(4.0))
    assert R.VARIANCE_DEFAULTS == VO.DEFAULTS
    d = R.variance_params()
    assert bytes(d) == bytes(p)
    assert hip_lib.rtHipVarianceScratchBytes(130, 70) == 68 * 130 * 70
    assert hip_lib.rtHipVarianceScratchBytes(0, 70) == 0 and hip_lib.rtHipVarianceScratchBytes(1 << 14, (1 << 13) + 1) == 0


BAD_VARIANCE = (dict(iterations=13), dict(luminance_sigma2=-1.0), dict(luminance_sigma2=np.nan), dict(luminance_sigma2=np.inf),
                dict(variance_floor=0.0), dict(variance_floor=2.0 ** -101), dict(variance_floor=np.nan), dict(variance_floor=np.inf),
                dict(albedo_inv_sigma2=-1.0), dict(albedo_inv_sigma2=np.inf), dict(normal_power_log2=11), dict(spatial_below=-1.0),
                dict(spatial_below=65538.0), dict(spatial_below=np.nan), dict(spatial_below=np.inf))
FIELD_OF = dict(iterations="iterations", luminance_sigma2="luminanceSigma2", variance_floor="varianceFloor", albedo_inv_sigma2="albedoInvSigma2",
                normal_power_log2="normalPowerLog2", spatial_below="spatialBelow")


def test_null_arguments_and_bad_parameters_are_refused_without_a_device():
    """(Nothing here reaches a device: the parameters and the NULL checks come first.)"""
    L = R.lib()
    W, H = 4, 3
    f = [np.full((H, W, 3), -3.0, F32) for _ in range(13)]
    ptr = [a.ctypes.data_as(C.c_void_p) for a in f]
    tp, vp = R.temporal_params(), R.variance_params()
    # the scene call
    assert L.rtHipSceneTemporalVariance(None, C.byref(tp), None, ptr[0], None, None, None, None, None) == -1 and "null" in R.last_error()
    # (a): 13 arrays; outCount (index 10) and outVariance (12) may be NULL
    for call, tail in ((L.rtHipTemporalMoments, ()), (L.rtHipTemporalMomentsDevice, (None,))):
        assert call(0, W, H, *ptr, None, *tail) == -1 and "null parameters" in R.last_error()
        for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11):
            args = list(ptr)
            args[i] = None
            assert call(0, W, H, *args, C.byref(tp), *tail) == -1 and "null array" in R.last_error(), i
        for bad in (dict(max_history=0.5), dict(max_history=np.nan), dict(depth_tolerance=-0.01), dict(depth_tolerance=np.inf)):
            assert call(0, W, H, *ptr, C.byref(R.temporal_params(**bad)), *tail) == -1, bad
            assert ("maxHistory" if "max_history" in bad else "depthTolerance") in R.last_error()
        for w, h in ((0, 3), (4, 0), (16385, 1), (1, 16385)):
            assert call(0, w, h, *ptr, C.byref(tp), *tail) == -1 and "image" in R.last_error(), (w, h)
    # (b), (c): colour normal albedo moments count out outVariance [scratch bytes]
    host = lambda params, *a: L.rtHipDenoiseVariance(0, W, H, *a, params)  # noqa: E731
    device = lambda params, *a: L.rtHipDenoiseVarianceDevice(0, W, H, *a, ptr[7], 68 * W * H, params, None)  # noqa: E731
    for call in (host, device):
        assert call(None, *ptr[:7]) == -1 and "null parameters" in R.last_error()
        for i in (0, 1, 2, 5):
            args = list(ptr[:7])
            args[i] = None
            assert call(C.byref(vp), *args) == -1 and "null array" in R.last_error(), i
        for i in (3, 4):  # moments without count, count without moments
            args = list(ptr[:7])
            args[i] = None
            assert call(C.byref(vp), *args) == -1 and "both NULL or both given" in R.last_error(), i
        for bad in BAD_VARIANCE:
            assert call(C.byref(R.variance_params(**bad)), *ptr[:7]) == -1, bad
            assert FIELD_OF[next(iter(bad))] in R.last_error(), (bad, R.last_error())
    assert L.rtHipDenoiseVarianceDevice(0, W, H, *ptr[:7], None, 68 * W * H, C.byref(vp), None) == -1 and "null array" in R.last_error()
    assert L.rtHipDenoiseVarianceDevice(0, W, H, *ptr[:7], ptr[7], 68 * W * H - 1, C.byref(vp), None) == -1 and "scratch" in R.last_error()
    for w, h in ((0, 3), (4, 0), (1 << 14, (1 << 13) + 1)):
        assert L.rtHipDenoiseVariance(0, w, h, *ptr[:7], C.byref(vp)) == -1 and "image" in R.last_error(), (w, h)
    assert all((a == -3.0).all() for a in f)
    with pytest.raises(ValueError):
        R.denoise_variance(f[0], f[1], f[2], moments=f[3][..., :2].copy())  # moments without count
    with pytest.raises(ValueError):
        R.temporal_moments(f[0], f[1][..., :2].copy(), f[2][..., 0].copy(), np.zeros((H, W), np.uint32), TO.empty_history(H, W))  # no moments


# ---- the kernels' per-pixel code, compiled for the host --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tests/variance_host.cpp (csrc/rt_variance_pixel.h, what the kernels of rt_variance.hip run per lane) as a host library."""
    out = tmp_path_factory.mktemp("variance_host") / "libvariance_host.so"
    subprocess.run([os.environ.get("CXX", "g++")] + HOST_FLAGS + ["-I", os.path.join(ROOT, "opencl_render_amd", "csrc"), "-o", str(out),
                    os.path.join(ROOT, "tests", "variance_host.cpp")], check=True)
    lib = C.CDLL(str(out))
    lib.variance_host_moments.restype = None
    lib.variance_host_moments.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 13 + [C.c_float, C.c_float]
    lib.variance_host_filter.restype = None
    lib.variance_host_filter.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_float]

    def moments(colour, motion, prev_t, triangle, history, max_history=TO.DEFAULTS["max_history"], depth_tolerance=TO.DEFAULTS["depth_tolerance"]):
        H, W = prev_t.shape
        ins = [np.ascontiguousarray(a) for a in (colour, motion, prev_t, triangle, history["colour"], history["count"], history["t"],
                                                 history["triangle"], history["moments"])]
        out = dict(colour=np.full((H, W, 3), -7.0, F32), count=np.full((H, W), -7.0, F32), moments=np.full((H, W, 2), -7.0, F32),
                   variance=np.full((H, W), -7.0, F32))
        lib.variance_host_moments(W, H, *[a.ctypes.data for a in ins], *[out[k].ctypes.data for k in ("colour", "count", "moments", "variance")],
                                  max_history, depth_tolerance)
        return out

    def filt(colour, normal, albedo, moments=None, count=None, **params):
        p = dict(VO.DEFAULTS, **params)
        H, W, _ = colour.shape
        ins = [np.ascontiguousarray(a) if a is not None else None for a in (colour, normal, albedo, moments, count)]
        out, var = np.full((H, W, 3), -7.0, F32), np.full((H, W), -7.0, F32)
        lib.variance_host_filter(W, H, *[a.ctypes.data if a is not None else None for a in ins], out.ctypes.data, var.ctypes.data,
                                 p["iterations"], p["luminance_sigma2"], p["variance_floor"], p["albedo_inv_sigma2"], p["normal_power_log2"],
                                 p["spatial_below"])
        return out, var

    return moments, filt


def assert_same(got, want, label):
    bad = np.flatnonzero(~VO.same_bits(got, want).reshape(-1))
    assert bad.size == 0, (f"{label}: differs in {bad.size} of {want.size} values; first {bad[:4]}: got {np.asarray(got).reshape(-1)[bad[:4]]}, "
                           f"want {np.asarray(want).reshape(-1)[bad[:4]]}")


@pytest.mark.parametrize("W, H", VC.SIZES)
def test_the_kernels_pixel_code_on_the_host_equals_the_oracle_bit_for_bit(host, W, H):
    moments, filt = host
    fields = VC.moment_fields(W, H)
    for params in ({}, dict(max_history=4.0, depth_tolerance=0.0), dict(max_history=1.0), dict(max_history=65536.0, depth_tolerance=0.3)):
        want, got = VO.accumulate(*fields, **params), moments(*fields, **params)
        for k in ("colour", "count", "moments", "variance"):
            assert_same(got[k], want[k], f"{W}x{H} {params}: {k}")
    f = VC.filter_fields(W, H)
    for params in FILTER_PARAMS + ((dict(iterations=8),) if (W, H) == VC.SIZES[-1] else ()):
        for single in (False, True):
            args = (f["colour"], f["normal"], f["albedo"]) + ((None, None) if single else (f["moments"], f["count"]))
            want_c, want_v = VO.denoise(*args, **params)
            got_c, got_v = filt(*args, **params)
            assert_same(got_c, want_c, f"{W}x{H} {params} single={single}: colour")
            assert_same(got_v, want_v, f"{W}x{H} {params} single={single}: variance")
            if params.get("iterations") == 0:
                assert_same(got_v, VO.estimate(*args, spatial_below=VO.DEFAULTS["spatial_below"]), "K = 0 returns V^0")
                assert got_c.tobytes() == f["colour"].tobytes()


# ---- known answers, exact -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", TC.SIZES)
def test_the_moments_calls_colour_and_count_equal_the_temporal_accumulation(W, H):
    fields = VC.moment_fields(W, H)
    plain = TC.fields(W, H)
    for params in ({}, dict(max_history=4.0, depth_tolerance=0.0), dict(max_history=1.0)):
        got, want = VO.accumulate(*fields, **params), TO.accumulate(*plain, **params)
        assert_same(got["colour"], want["colour"], f"{W}x{H} {params}: colour")
        assert_same(got["count"], want["count"], f"{W}x{H} {params}: count")


def smooth_guides(W, H, seed=3):
    """Normals within a narrow cone and albedos close together: every tap's weight is > 0 (an infinite variance times a zero weight is a
    NaN, by definition; with positive weights the variance stays +inf through the iterations)."""
    rng = np.random.default_rng(seed)
    normal = np.concatenate([0.2 * rng.random((H, W, 2)) - 0.1, np.ones((H, W, 1))], -1).astype(F32)
    albedo = (0.4 + 0.2 * rng.random((H, W, 3))).astype(F32)
    return rng.random((H, W, 3), dtype=F32), normal, albedo


def test_an_infinite_variance_gives_the_denoiser_without_its_colour_edge_stop():
    W, H = 37, 29
    colour, normal, albedo = smooth_guides(W, H)
    inf = np.full((H, W), np.inf, F32)
    for K in (1, 3, 5):
        params = dict(iterations=K, albedo_inv_sigma2=30.0, normal_power_log2=2)
        got, v = VO.iterate(colour, inf, normal, albedo, luminance_sigma2=4.0, variance_floor=1e-8, **params)
        want = DO.denoise(colour, normal, albedo, colour_inv_sigma2=0.0, **params)
        assert got.tobytes() == want.tobytes() and np.isposinf(v).all(), K
        assert not np.array_equal(got, colour)
    # and through the estimate: m2 = +inf on the temporal arm is V^0 = +inf
    mom = np.stack([VO.lum(colour), inf], -1)
    got, _ = VO.denoise(colour, normal, albedo, mom, np.full((H, W), 8.0, F32), iterations=3, albedo_inv_sigma2=30.0, normal_power_log2=2)
    assert got.tobytes() == DO.denoise(colour, normal, albedo, iterations=3, colour_inv_sigma2=0.0, albedo_inv_sigma2=30.0, normal_power_log2=2).tobytes()


def test_a_flat_image_keeps_its_colour_and_its_unit_variance_shrinks_to_4900_65536ths():
    W, H = 11, 9
    colour = np.broadcast_to(F32([0.25, 0.5, 0.8125]), (H, W, 3)).copy()
    normal = np.broadcast_to(F32([0.0, 0.0, 2.0]), (H, W, 3)).copy()
    albedo = np.full((H, W, 3), 0.5, F32)
    c1, v1 = VO.iterate(colour, np.ones((H, W), F32), normal, albedo, iterations=1)
    assert c1.tobytes() == colour.tobytes()
    assert (v1[2:-2, 2:-2] == F32(4900.0 / 65536.0)).all() and F32(4900.0 / 65536.0) == 4900.0 / 65536.0
    assert (v1[0, 0] > v1[2, 2]) and np.isfinite(v1).all()  # fewer taps at the border: less averaging


def test_constant_frames_give_variance_exactly_zero():
    colour, motion, t, tri = still(value=(0.3, 0.6, 0.9))  # (a luminance that is not exact in fp32)
    H, W = t.shape
    hist = VO.empty_history(H, W)
    for n in range(1, 12):
        out = VO.accumulate(colour, motion, t, tri, hist, max_history=8.0)
        assert (out["variance"] == 0.0).all() and (out["count"] == F32(min(n, 8))).all(), n
        assert out["colour"].tobytes() == colour.tobytes()
        hist = VO.next_history(out, t, tri)
    # so the temporal arm of the estimate is 0 too; only the spatial arm sees a single frame's noise
    normal, albedo = np.broadcast_to(F32([0, 0, 1]), (H, W, 3)).copy(), np.full((H, W, 3), 0.5, F32)
    assert (VO.estimate(colour, normal, albedo, out["moments"], out["count"]) == 0.0).all()


# ---- the GPU tests' inputs are not vacuous ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", VC.SIZES[1:])
def test_the_filter_fields_take_both_arms_and_the_filter_changes_them(W, H):
    f = VC.filter_fields(W, H)
    spatial, temporal, positive, changed = VC.shares(f)
    print(f"{W} x {H}: spatial arm {spatial:.3f}, temporal arm {temporal:.3f}, V^0 > 0 {positive:.3f}, changed {changed:.3f}")
    assert spatial >= VC.MIN_ARM and temporal >= VC.MIN_ARM and positive >= VC.MIN_POSITIVE and changed >= VC.MIN_CHANGED
    sp = VC.special_pixels(W, H)
    assert sorted(sp) == sorted(VC.SPECIALS) and len(set(sp.values())) == len(sp)
    at = lambda k, name: f[k][sp[name]]  # noqa: E731
    assert np.isnan(at("colour", "NaN colour")).all() and at("count", "count 0") == 0 and np.isnan(at("count", "count NaN"))
    assert np.isposinf(at("count", "count inf")) and np.isposinf(at("moments", "infinite m1")[0]) and np.isposinf(at("moments", "infinite m2")[1])
    m = at("moments", "m2 < m1^2")
    assert m[1] < m[0] * m[0] and (at("normal", "zero normal") == 0).all()


@pytest.mark.parametrize("W, H", VC.SIZES[1:])
def test_the_moment_fields_hold_their_specials(W, H):
    hist = VC.moment_fields(W, H)[4]
    m1, m2 = hist["moments"][..., 0], hist["moments"][..., 1]
    with np.errstate(all="ignore"):
        assert (m2 < m1 * m1).any() and np.isposinf(m2).any() and np.isinf(m1).any() and np.isnan(m1).any()
    out = VO.accumulate(*VC.moment_fields(W, H))
    assert (out["variance"] > 0).mean() > 0.5 and (out["variance"] == 0).any() and np.isnan(out["moments"]).any()
