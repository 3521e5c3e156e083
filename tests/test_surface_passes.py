"""Surface passes, the parts that need no GPU: the colour PFM sink byte for byte, the command line's --surface-passes and the new
symbols of the C ABI."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT
from opencl_render_amd import __main__ as cli, frontend as F, raytrace as R

NEW_SYMBOLS = ["rtHipSurfaceBuffer", "rtHipSurfaceBufferBytes", "rtHipReadbackSurfacePasses", "rtHipWritePfmRgb"]


def test_pfm_rgb_sink_writes_interleaved_little_endian_floats_bottom_row_first(tmp_path):
    img = np.array([[[1.0, -2.5, 0.0], [np.inf, -0.0, 3.25]],
                    [[1e-30, 0.5, -1.0], [7.0, 8.0, 9.0]],
                    [[np.nan, 1.0, 2.0], [0.25, 0.125, 1e30]]], np.float32)  # [H=3, W=2, 3]
    path = str(tmp_path / "n.pfm")
    F.write_pfm_rgb(path, img)
    rows = [struct.pack("<6f", *img[r].ravel().tolist()) for r in (2, 1, 0)]
    raw = open(path, "rb").read()
    assert raw == b"PF\n2 3\n-1.0\n" + b"".join(rows)


def test_pfm_rgb_sink_keeps_every_bit(tmp_path):
    rng = np.random.default_rng(11)
    img = (rng.standard_normal((5, 7, 3)) * 100).astype(np.float32)
    path = str(tmp_path / "a.pfm")
    F.write_pfm_rgb(path, img)
    raw = open(path, "rb").read()
    head = b"PF\n7 5\n-1.0\n"
    back = np.frombuffer(raw[len(head):], "<f4").reshape(5, 7, 3)[::-1]
    assert raw.startswith(head) and np.array_equal(back.view(np.uint32), img.view(np.uint32))


def test_pfm_rgb_sink_refuses_bad_arguments(tmp_path):
    L = R.lib()
    L.rtHipWritePfmRgb.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
    img = np.zeros((2, 2, 3), np.float32)
    assert L.rtHipWritePfmRgb(str(tmp_path / "x.pfm").encode(), 2, 2, None) == -1
    assert L.rtHipWritePfmRgb(str(tmp_path / "x.pfm").encode(), 0, 2, img.ctypes.data_as(C.c_void_p)) == -1
    assert L.rtHipWritePfmRgb(str(tmp_path / "no" / "x.pfm").encode(), 2, 2, img.ctypes.data_as(C.c_void_p)) == -4
    with pytest.raises(ValueError):
        F.write_pfm_rgb(str(tmp_path / "y.pfm"), np.zeros((2, 2), np.float32).reshape(2, 2, 1))


def test_command_line_accepts_surface_passes_only_with_passes(capsys):
    args = cli.parse_args(["--scene", "soup", "--passes", "out/frame", "--surface-passes"])
    assert args.passes == "out/frame" and args.surface_passes
    assert not cli.parse_args(["--passes", "out/frame"]).surface_passes
    with pytest.raises(SystemExit):
        cli.parse_args(["--surface-passes"])
    assert "--surface-passes needs --passes" in capsys.readouterr().err


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in R.RESIDENT_SYMBOLS, name
        assert hasattr(R.lib(), name), name
    assert re.search(r"#define RT_HIP_PASS_NORMAL\s+8u", header) and R.PASS_NORMAL == 8
    assert re.search(r"#define RT_HIP_PASS_ALBEDO\s+16u", header) and R.PASS_ALBEDO == 16
