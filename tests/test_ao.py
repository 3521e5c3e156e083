"""Ambient occlusion without a GPU: the C ABI declares and exports the AO entry points with their parameter record and defaults, and
the numpy restatement (ao_oracle.py, walks by rt_oracle_grid_trace) behaves as the definition says -- splitmix64's known outputs,
cosine-weighted directions in the normal's hemisphere, nothing occludes a lone triangle, a closed box occludes everything, a miss is
open.  The device is checked against the same restatement in test_ao_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ao_oracle as A
from conftest import ROOT
from opencl_render_amd import raytrace as R, scene as S

F32 = np.float32


def mesh_scene(width, height, verts, tris, name):
    """The soup's camera (eye at the origin looking along +z) over the given triangles, lists built on the host."""
    sc = S.make_soup(width, height, 1, 0.01, seed=1, name=name)
    T = len(tris)
    sc.vertex = np.zeros((len(verts), 4), F32)
    sc.vertex[:, :3] = verts
    sc.tri_index = np.zeros((T, 4), np.int32)
    sc.tri_index[:, :3] = tris
    sc.tri_material = np.zeros(T, np.int32)
    sc.tri_uv = np.zeros((3 * T, 2), F32)
    sc.tri_normal = np.zeros((3 * T, 4), F32)
    sc.tri_normal[:, 2] = -1.0
    R.build_lists(sc)
    return sc


def one_triangle():
    """One big triangle facing the camera at z = 3; the image's corners miss it."""
    return mesh_scene(48, 36, [(-1.0, -1.0, 3.0), (1.0, -1.0, 3.0), (0.0, 1.0, 3.0)], [(0, 1, 2)], "ao_one_triangle")


def closed_box():
    """The eye inside a closed box (x, y in [-1, 1], z in [-1, 3]), 12 triangles."""
    v = [(x, y, z) for z in (-1.0, 3.0) for y in (-1.0, 1.0) for x in (-1.0, 1.0)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return mesh_scene(32, 24, v, tris, "ao_closed_box")


def test_header_declares_the_ao_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ("rtHipAoDefaults", "rtHipSceneAmbientOcclusion", "rtHipSceneAmbientOcclusionDevice"):
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert "AMBIENT OCCLUSION" in text
    assert C.sizeof(R.AoParams) == 16
    assert [f[0] for f in R.AoParams._fields_] == ["raysPerHit", "pixelSamples", "radius", "seed"]


def test_defaults_match_the_header():
    p = R.AoParams(1, 2, 3.0, 4)
    R.lib().rtHipAoDefaults(C.byref(p))
    assert (p.raysPerHit, p.pixelSamples, p.radius, p.seed) == (16, 1, np.inf, 0)
    assert R.AO_DEFAULTS == dict(rays=16, radius=np.inf, pixel_samples=1, seed=0)


def test_null_arguments_are_refused_without_a_device():
    L = R.lib()
    p = R.AoParams()
    L.rtHipAoDefaults(C.byref(p))
    out = np.zeros(4, F32)
    assert L.rtHipSceneAmbientOcclusion(None, C.byref(p), out.ctypes.data_as(C.c_void_p)) == -1
    assert "null" in R.last_error()
    assert L.rtHipSceneAmbientOcclusionDevice(None, C.byref(p), out.ctypes.data_as(C.c_void_p), None) == -1
    with pytest.raises(ValueError):
        R.ao_params(rays=-1)
    with pytest.raises(ValueError):
        R.ao_params(seed=1 << 32)


def test_splitmix64_anchors():
    h = A.hashes(0, np.arange(3))
    assert [int(x) for x in h] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    u = A.uniform(0, np.arange(3))
    assert u.dtype == F32 and np.array_equal(u, (h >> np.uint64(40)).astype(np.float64).astype(F32) / F32(1 << 24))
    with np.errstate(all="raise"):  # the array arithmetic wraps without a warning
        A.hashes(0xFFFFFFFF, np.arange(1000, dtype=np.uint64) * np.uint64(0x1234567890ABCDEF))


def test_directions_are_cosine_weighted_in_the_hemisphere():
    rng = np.random.default_rng(5)
    n = rng.normal(size=(20000, 3)).astype(F32)
    n[:8] = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, -1, 0), (1, 0, -0.0), (0.6, 0, -0.8), (0, 0.6, 0.8), (-1, 0, 0)]
    n /= np.sqrt((n * n).sum(1, keepdims=True))
    counters = (rng.integers(0, 1 << 40, (len(n), 8)) * 32).astype(np.uint64)
    d = A.hemisphere(n.astype(F32), counters, seed=9)
    cos = A.dot(d, n[:, None, :].astype(F32))
    assert cos.min() >= -1e-6
    assert abs(float(cos.mean()) - 2.0 / 3.0) < 0.005
    assert np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(-1)) - 1).max() < 1e-5


def test_a_lone_triangle_occludes_nothing():
    sc = one_triangle()
    img, rays = A.ambient_occlusion(sc, rays=8, pixel_samples=2, seed=3, with_rays=True)
    hit = np.zeros(sc.width * sc.height, bool)
    hit[rays["sample"] // 2] = True
    assert 0.3 < hit.mean() < 0.9  # hit pixels and missed pixels both present
    assert np.array_equal(img, np.ones((sc.height, sc.width), F32))


def test_a_closed_box_occludes_everything():
    sc = closed_box()
    img, rays = A.ambient_occlusion(sc, rays=16, with_rays=True)
    assert len(rays["sample"]) == 16 * sc.width * sc.height  # every pixel hits a wall
    assert float(img.mean()) < 0.02
    short = A.ambient_occlusion(sc, rays=16, radius=1e-3)  # almost nothing is that close
    assert float(short.mean()) > 0.9


def test_a_missed_pixel_is_open():
    sc = one_triangle()
    sc.eye_to_top_left = np.asarray(sc.eye_to_top_left, F32).copy()
    sc.eye_to_top_left[0] = F32(5.0)  # the whole view to the right of the triangle
    img, rays = A.ambient_occlusion(sc, rays=4, with_rays=True)
    assert len(rays["sample"]) == 0
    assert np.array_equal(img, np.ones_like(img))
