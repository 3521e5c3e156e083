"""Scene edits without a GPU (include/raytrace_hip.h, "SCENE EDITS: LIGHTS AND MATERIALS"): the entry points refuse NULL arguments with a
text, rtHipLightsCheck / rtHipMaterialsCheck decide a table of cases, the same arithmetic (csrc/rt_scene_edit.h) runs in a program of its
own -- tests/scene_edit_host.cpp, once as built and once under the address and undefined-behaviour sanitizers -- over that table and over
seeded random tables checked in 128-bit arithmetic, and raytrace.relight turns light 0 only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from opencl_render_amd import raytrace as R, scene as S

FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", os.path.join(ROOT, "include"),
         "-I", os.path.join(ROOT, "opencl_render_amd", "csrc")]


def test_symbols_are_declared_and_exported():
    L = R.lib()
    for name in ("rtHipLightsCheck", "rtHipMaterialsCheck", "rtHipSceneSetLights", "rtHipSceneSetMaterials", "rtHipSceneEditTimes"):
        assert name in R.RESIDENT_SYMBOLS
        assert getattr(L, name) is not None


def test_null_arguments_are_refused_with_a_text():
    L = R.lib()
    lights, update, ms = R.Lights(), R.MaterialUpdate(), (C.c_double * 3)()
    fake = C.c_void_p(16)  # (never dereferenced: the other argument is NULL)
    for call, text in ((lambda: L.rtHipSceneSetLights(None, C.byref(lights)), "rtHipSceneSetLights"),
                       (lambda: L.rtHipSceneSetLights(fake, None), "rtHipSceneSetLights"),
                       (lambda: L.rtHipSceneSetMaterials(None, C.byref(update)), "rtHipSceneSetMaterials"),
                       (lambda: L.rtHipSceneSetMaterials(fake, None), "rtHipSceneSetMaterials"),
                       (lambda: L.rtHipSceneEditTimes(None, C.byref(ms)), "rtHipSceneEditTimes"),
                       (lambda: L.rtHipLightsCheck(None), "lights"),
                       (lambda: L.rtHipMaterialsCheck(None), "materials")):
        L.rtHipTune(b"reset", 0.0)  # (any successful call: the text below is this call's own)
        assert call() == -1
        assert text in R.last_error() and "null" in R.last_error(), R.last_error()


def _lights(count, missing=None):
    a = dict(zip(R.LIGHT_FIELDS, S.pack_lights([dict(type=3)] * min(count, 2))))
    ptr = [R._ptr(a[k]) for k in R.LIGHT_FIELDS]  # (a check reads no array: two rows stand in for any count)
    if missing is not None:
        ptr[missing] = None
    return R.Lights(count, *ptr), a


LIGHT_CASES = [("65535 lights", 65535, None, None), ("65536 lights", 65536, None, "too large"), ("no lights, NULL arrays", 0, "all", None)] + \
              [(f"one light, NULL {R.LIGHT_FIELDS[i]}", 1, i, "null light array") for i in range(6)]


@pytest.mark.parametrize("label,count,missing,text", LIGHT_CASES, ids=[c[0] for c in LIGHT_CASES])
def test_lights_check(label, count, missing, text):
    arg, keep = (R.Lights(0), None) if missing == "all" else _lights(count, missing)
    rc = R.lib().rtHipLightsCheck(C.byref(arg))
    if text is None:
        assert rc == 0, R.last_error()
    else:
        assert rc == -1 and text in R.last_error(), (rc, R.last_error())


def _channel(w, h, start, texels):
    size, st = np.zeros((5, 2), np.uint32), np.zeros(5, np.int32)
    size[0], st[0] = (w, h), start
    tex = np.zeros((1, 4), np.uint8)  # (a check reads no texel)
    return R.MaterialUpdate(1, 1, R._ptr(size), R._ptr(st), texels, R._ptr(tex), None, 0), (size, st, tex)


MATERIAL_CASES = [
    ("w > 0 with start < 0", (2, 3, -1, 100), "exceed"),
    ("absent channel with start < 0", (0, 3, -1, 100), None),
    ("start + w*h == texturesSize", (4, 5, 80, 100), None),
    ("start + w*h == texturesSize + 1", (4, 5, 81, 100), "exceed"),
    ("w = h = 0xffffffff", (0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF), "exceed"),
    ("w = h = 65536", (65536, 65536, 0, 0xFFFFFFFF), "exceed"),
    ("w > 0, h = 0", (7, 0, 100, 100), None),
    ("w > 0, h = 0 past the atlas", (7, 0, 101, 100), "exceed"),
]


@pytest.mark.parametrize("label,channel,text", MATERIAL_CASES, ids=[c[0] for c in MATERIAL_CASES])
def test_materials_check(label, channel, text):
    arg, keep = _channel(*channel)
    rc = R.lib().rtHipMaterialsCheck(C.byref(arg))
    if text is None:
        assert rc == 0, R.last_error()
    else:
        assert rc == -1 and text in R.last_error(), (rc, R.last_error())


def test_materials_check_needs_tables_or_ids():
    L = R.lib()
    assert L.rtHipMaterialsCheck(C.byref(R.MaterialUpdate())) == -1 and "neither" in R.last_error()
    ids = np.zeros(3, np.int32)
    assert L.rtHipMaterialsCheck(C.byref(R.MaterialUpdate(0, 0, None, None, 0, None, R._ptr(ids), 0))) == 0
    assert L.rtHipMaterialsCheck(C.byref(R.MaterialUpdate(1, 0, None, None, 0, None, None, 0))) == 0  # no materials at all
    assert L.rtHipMaterialsCheck(C.byref(R.MaterialUpdate(1, 2, None, None, 0, None, None, 0))) == -1 and "null material table" in R.last_error()


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run([os.environ.get("CXX", "g++")] + extra + FLAGS + ["-o", str(out), os.path.join(ROOT, "tests", "scene_edit_host.cpp")], check=True)
    return str(out)


def _run(program, *args):
    done = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr or done.stdout
    return done.stdout


def test_host_program_known_answers_and_random_tables(tmp_path_factory):
    out = _run(_build(tmp_path_factory, "scene_edit_host", ["-O2"]), 1, 4000)
    assert "failures 0" in out


def test_host_program_under_address_and_undefined_sanitizers(tmp_path_factory):
    program = _build(tmp_path_factory, "scene_edit_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = _run(program, 2, 3000)
    assert "failures 0" in out


def test_relight_turns_light_zero_only():
    lights = [dict(type=S.LIGHT_SPOT, pos=(0.4, 0.6, 1.5), dir=(0.3, -0.8, 0.5), col=(0.9, 0.8, 0.7), radius=0.2, half_att=2.0),
              dict(type=S.LIGHT_DISTANT, pos=(1, 2, 3), dir=(-0.5, 0.1, 0.2)), dict(type=S.LIGHT_AREA, pos=(-0.8, -0.3, 2.5), radius=0.05)]
    a = dict(zip(R.LIGHT_FIELDS, S.pack_lights(lights)))
    same = R.relight(a, 0, 5)
    assert set(same) == set(R.LIGHT_FIELDS)
    for k in R.LIGHT_FIELDS:
        assert same[k].tobytes() == a[k].tobytes() and same[k].dtype == a[k].dtype and same[k] is not a[k], k
    assert all(R.relight(a, 5, 5)[k].tobytes() == a[k].tobytes() for k in R.LIGHT_FIELDS)  # a whole turn is pose 0
    for k in (1, 2, 4):
        out = R.relight(a, k, 5)
        for name in R.LIGHT_FIELDS:
            assert out[name][1:].tobytes() == a[name][1:].tobytes(), name  # lights 1.. untouched
        for name in ("light_type", "light_col", "light_radius", "light_half_att"):
            assert out[name].tobytes() == a[name].tobytes(), name
        for name in ("light_pos", "light_dir"):
            assert out[name].dtype == np.float32 and out[name][0, 1] == a[name][0, 1] and out[name][0, 3] == 0  # the height stays
            assert not np.array_equal(out[name][0], a[name][0])
            before, after = np.hypot(a[name][0, 0], a[name][0, 2]), np.hypot(out[name][0, 0], out[name][0, 2])
            assert abs(before - after) < 1e-6  # a turn keeps the distance to the axis
    quarter = R.relight(a, 1, 4)  # x' = z, z' = -x up to the rounding of cos(pi/2) in float32
    assert np.allclose(quarter["light_dir"][0, :3], [0.5, -0.8, -0.3], atol=1e-6)
    empty = dict(zip(R.LIGHT_FIELDS, S.pack_lights([])))
    assert R.relight(empty, 1, 3)["light_type"].shape == (0,)
