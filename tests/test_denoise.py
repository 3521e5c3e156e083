"""The denoiser, the parts that need no GPU: properties of the numpy oracle (tests/denoise_oracle.py), the new C ABI symbols, parameter
validation before anything is launched, the scratch size and the command line's --denoise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_oracle as D
from conftest import ROOT
from opencl_render_amd import __main__ as cli, raytrace as R

NEW_SYMBOLS = ["rtHipDenoiseDefaults", "rtHipDenoiseScratchBytes", "rtHipDenoiseDevice", "rtHipDenoise", "rtHipSceneDenoise",
               "rtHipSceneDenoiseTimes"]


def random_inputs(H, W, seed):
    rng = np.random.default_rng(seed)
    colour = rng.random((H, W, 3), dtype=np.float32)
    normal = rng.standard_normal((H, W, 3)).astype(np.float32)
    albedo = rng.random((H, W, 3), dtype=np.float32)
    return colour, normal, albedo


def test_zero_iterations_is_the_identity():
    c, n, a = random_inputs(9, 11, 1)
    c[0, 0] = [np.nan, np.inf, -0.0]
    out = D.denoise(c, n, a, iterations=0)
    assert out.dtype == np.float32 and out.view(np.uint32).tobytes() == c.view(np.uint32).tobytes()


def test_halves_with_orthogonal_normals_never_mix():
    H, W = 12, 16
    c, _, a = random_inputs(H, W, 2)
    c[:, : W // 2] *= np.float32(0.25)
    c[:, W // 2:] += np.float32(3.0)
    n = np.zeros((H, W, 3), np.float32)
    n[:, : W // 2] = [0, 0, 2]   # not normalised on purpose: the guides normalise
    n[:, W // 2:] = [1, 0, 0]
    out = D.denoise(c, n, a, iterations=5, colour_inv_sigma2=0.0, albedo_inv_sigma2=0.0, normal_power_log2=0)
    left, right = out[:, : W // 2], out[:, W // 2:]
    assert left.max() <= c[:, : W // 2].max() and left.min() >= c[:, : W // 2].min()
    assert right.min() >= c[:, W // 2:].min() and right.max() <= c[:, W // 2:].max()
    # the same filter on the left half alone gives the same left half: no weight crossed the edge
    alone = D.denoise(np.ascontiguousarray(c[:, : W // 2]), np.ascontiguousarray(n[:, : W // 2]), np.ascontiguousarray(a[:, : W // 2]),
                      iterations=5, colour_inv_sigma2=0.0, albedo_inv_sigma2=0.0, normal_power_log2=0)
    assert np.array_equal(alone.view(np.uint32), left.view(np.uint32))


def test_a_constant_image_stays_within_a_few_ulps():
    H, W = 40, 50
    _, n, a = random_inputs(H, W, 3)
    value = np.float32(0.3719)
    c = np.full((H, W, 3), value, np.float32)
    out = D.denoise(c, n, a, iterations=5)
    ulps = np.abs(out.view(np.int32).astype(np.int64) - c.view(np.int32).astype(np.int64))
    assert ulps.max() <= 32, ulps.max()


def test_no_edge_stopping_with_zero_normals_is_the_plain_b3_atrous_blur():
    H, W = 13, 17
    c, _, a = random_inputs(H, W, 4)
    n = np.zeros((H, W, 3), np.float32)
    out = D.denoise(c, n, a, iterations=2, colour_inv_sigma2=0.0, albedo_inv_sigma2=0.0)
    # the textbook a-trous blur, written independently: normalised 5x5 B3 stencil with holes, skipped taps outside the image, float64
    ref = c.astype(np.float64)
    b = np.array([1, 4, 6, 4, 1], np.float64) / 16
    for i in range(2):
        h = 1 << i
        acc = np.zeros_like(ref)
        wsum = np.zeros((H, W), np.float64)
        for j in range(5):
            for k in range(5):
                dy, dx = (j - 2) * h, (k - 2) * h
                for y in range(H):
                    for x in range(W):
                        if 0 <= y + dy < H and 0 <= x + dx < W:
                            acc[y, x] += b[j] * b[k] * ref[y + dy, x + dx]
                            wsum[y, x] += b[j] * b[k]
        ref = acc / wsum[..., None]
    assert np.allclose(out, ref, rtol=2e-6, atol=1e-7)


def test_the_oracle_refuses_other_dtypes():
    c, n, a = random_inputs(3, 3, 5)
    with pytest.raises(AssertionError, match="float32"):
        D.denoise(c.astype(np.float64), n, a)


def test_quantise_follows_the_rounding_rule():
    v = np.array([[[-1.0, 0.0, np.nan], [1.0, 2.0, np.inf], [0.5 / 65535, 0.49 / 65535, 65534.49 / 65535]]], np.float32)
    r, g, b = D.quantise(v)
    assert r.tolist() == [[0, 65535, 1]] and g.tolist() == [[0, 65535, 0]] and b.tolist() == [[0, 65535, 65534]]
    for x, y in zip(D.quantise(v), R.quantise(v)):
        assert np.array_equal(x, y)


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    L = R.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in R.RESIDENT_SYMBOLS, name
        assert hasattr(L, name), name


def test_defaults_agree_between_the_library_and_python():
    p = R.DenoiseParams()
    R.lib().rtHipDenoiseDefaults(C.byref(p))
    assert (p.iterations, p.colourInvSigma2, p.albedoInvSigma2, p.normalPowerLog2) == (
        R.DENOISE_DEFAULTS["iterations"], R.DENOISE_DEFAULTS["colour_inv_sigma2"], R.DENOISE_DEFAULTS["albedo_inv_sigma2"],
        R.DENOISE_DEFAULTS["normal_power_log2"])


@pytest.mark.parametrize("params, text", [
    (dict(iterations=13), "iterations 13"),
    (dict(colour_inv_sigma2=float("nan")), "colourInvSigma2"),
    (dict(colour_inv_sigma2=-1.0), "colourInvSigma2"),
    (dict(colour_inv_sigma2=float("inf")), "colourInvSigma2"),
    (dict(albedo_inv_sigma2=float("nan")), "albedoInvSigma2"),
    (dict(albedo_inv_sigma2=-0.5), "albedoInvSigma2"),
    (dict(normal_power_log2=11), "normalPowerLog2"),
    (dict(iterations=12, colour_inv_sigma2=3e32), "overflows"),  # 3e32 * 4^11 = 1.3e39 > FLT_MAX
])
def test_bad_parameters_are_refused_before_anything_runs(params, text):
    L = R.lib()
    p = R.denoise_params(**params)
    img = np.zeros((2, 3, 3), np.float32)
    ptr = img.ctypes.data_as(C.c_void_p)
    assert L.rtHipDenoise(0, 3, 2, ptr, ptr, ptr, ptr, C.byref(p)) == -1
    assert text in R.last_error()
    assert L.rtHipDenoiseDevice(0, 3, 2, ptr, ptr, ptr, ptr, ptr, 1 << 20, C.byref(p), None) == -1
    assert text in R.last_error()
    assert L.rtHipSceneDenoise(None, C.byref(p), None, None, None, None) == -1
    with pytest.raises(RuntimeError, match=text):
        R.denoise(img, img, img, **params)


@pytest.mark.parametrize("params", [dict(iterations=2 ** 32 + 1), dict(normal_power_log2=2 ** 32), dict(iterations=-1)])
def test_python_refuses_integers_outside_the_uint32_fields(params):
    with pytest.raises(ValueError, match="0..2\\^32-1"):
        R.denoise_params(**params)
    img = np.zeros((2, 2, 3), np.float32)
    with pytest.raises(ValueError):
        R.denoise(img, img, img, **params)


def test_scene_denoise_times_refuse_null_arguments():
    ms = (C.c_float * 3)()
    assert R.lib().rtHipSceneDenoiseTimes(None, ms) == -1


def test_the_variant_build_links_the_makefiles_objects():
    """scripts/build_variant.sh relinks the library with a variant rt_wavefront object: it must take every other object from the
    Makefile's OBJS (a hand-written list once left out rt_denoise.o and its libraries failed to load)."""
    import subprocess
    csrc = os.path.join(ROOT, "opencl_render_amd", "csrc")
    objs = subprocess.run(["make", "-s", "objs"], cwd=csrc, capture_output=True, text=True, check=True).stdout.split()
    sources = sorted(os.path.splitext(f)[0] for f in os.listdir(csrc) if f.endswith((".hip", ".cpp")))
    assert sorted(os.path.splitext(os.path.basename(o))[0] for o in objs) == sources
    script = open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()
    assert "make -s objs" in script and "rt_api.o" not in script


def test_largest_colour_sigma_that_does_not_overflow_is_accepted_by_validation():
    L = R.lib()
    p = R.denoise_params(iterations=12, colour_inv_sigma2=float(np.finfo(np.float32).max / np.float32(4.0 ** 11)))
    # validation passes, so the call gets as far as the size check
    assert L.rtHipDenoiseDevice(0, 0, 2, None, None, None, None, None, 0, C.byref(p), None) == -1
    assert "1..2^27 pixels" in R.last_error()


def test_bad_sizes_are_refused():
    L = R.lib()
    p = R.denoise_params()
    for w, h in ((0, 5), (5, 0), (1 << 14, (1 << 13) + 1)):
        assert L.rtHipDenoise(0, w, h, None, None, None, None, C.byref(p)) == -1
        assert "1..2^27 pixels" in R.last_error()


def test_scratch_bytes():
    L = R.lib()
    assert L.rtHipDenoiseScratchBytes(1, 1) == 64
    assert L.rtHipDenoiseScratchBytes(1920, 1080) == 1920 * 1080 * 64
    assert L.rtHipDenoiseScratchBytes(1 << 14, 1 << 13) == (1 << 27) * 64
    assert L.rtHipDenoiseScratchBytes(1 << 14, (1 << 13) + 1) == 0
    assert L.rtHipDenoiseScratchBytes(0, 7) == 0 and L.rtHipDenoiseScratchBytes(7, 0) == 0


def test_command_line_denoise(capsys):
    args = cli.parse_args(["--scene", "room", "--denoise", "out/den.pfm"])
    assert args.denoise == "out/den.pfm" and not args.passes
    assert cli.parse_args(["--denoise", "a.BMP", "--passes", "p", "--surface-passes"]).denoise == "a.BMP"
    assert cli.parse_args(["--denoise", "a.ppm"]).denoise == "a.ppm"
    assert cli.parse_args([]).denoise is None
    with pytest.raises(SystemExit):
        cli.parse_args(["--denoise", "a.png"])
    assert "--denoise PATH must end in .bmp, .ppm or .pfm" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_args(["--denoise"])
