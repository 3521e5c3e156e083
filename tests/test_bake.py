"""The ambient occlusion bake without a GPU: the C ABI declares and exports the bake's entry points with their parameter record and
defaults, refuses null arguments, and the numpy restatement (bake_oracle.py, walks by rt_oracle_grid_trace) behaves as the definition
says -- coverage of a unit quad, the smallest id on a shared edge, nothing from degenerate or NaN UVs, a lone triangle open, a closed box
occluded, the dilation on hand-made maps -- and scene.grid_atlas_uv gives every triangle a cell of its own.  The device is checked
against the same restatement in test_bake_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bake_oracle as B
from conftest import ROOT
from opencl_render_amd import raytrace as R, scene as S
from test_ao import mesh_scene

F32 = np.float32
NONE = 0xFFFFFFFF


def with_uv(sc, uv):
    sc.tri_uv = np.ascontiguousarray(np.asarray(uv, F32).reshape(-1, 2))
    return sc


def quad(w=8, h=8):
    """A unit square facing the camera at z = 3, two triangles sharing the diagonal, UVs over [0, 1]^2."""
    sc = mesh_scene(w, h, [(-1.0, -1.0, 3.0), (1.0, -1.0, 3.0), (-1.0, 1.0, 3.0), (1.0, 1.0, 3.0)], [(0, 1, 2), (3, 2, 1)], "bake_quad")
    return with_uv(sc, [(0, 0), (1, 0), (0, 1), (1, 1), (0, 1), (1, 0)])


def closed_box(inward=True):
    """A closed box (x, y in [-1, 1], z in [-1, 3]), 12 triangles on a grid atlas, corner normals pointing in (or out)."""
    v = np.array([(x, y, z) for z in (-1.0, 3.0) for y in (-1.0, 1.0) for x in (-1.0, 1.0)], F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    sc = mesh_scene(16, 16, v, tris, "bake_closed_box")
    centre = v.mean(0)
    n = np.zeros((len(tris), 3, 4), F32)
    for i, t in enumerate(tris):
        d = centre - v[list(t)].mean(0)
        n[i, :, :3] = d if inward else -d
    sc.tri_normal = np.ascontiguousarray(n.reshape(-1, 4))
    return with_uv(sc, S.grid_atlas_uv(len(tris), 32, margin_texels=1.3))


def test_header_declares_the_bake_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ("rtHipBakeDefaults", "rtHipSceneBakeAmbientOcclusion", "rtHipSceneBakeAmbientOcclusionDevice"):
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert "AMBIENT OCCLUSION BAKE" in text and '"bake_texels"' in text
    assert C.sizeof(R.BakeParams) == 40
    assert [f[0] for f in R.BakeParams._fields_] == ["width", "height", "raysPerTexel", "radius", "seed", "dilate", "firstTriangle",
                                                     "triangleCount", "material", "matchMaterial"]


def test_defaults_match_the_header():
    p = R.BakeParams(*range(1, 11))
    R.lib().rtHipBakeDefaults(C.byref(p))
    assert (p.width, p.height, p.raysPerTexel, p.radius, p.seed, p.dilate) == (0, 0, 16, np.inf, 0, 2)
    assert (p.firstTriangle, p.triangleCount, p.matchMaterial) == (0, 0xFFFFFFFF, 0)
    assert R.BAKE_DEFAULTS == dict(rays=16, radius=np.inf, seed=0, dilate=2)
    q = R.bake_params(7, 5, triangles=range(3, 9), material=-1)
    assert (q.width, q.height, q.firstTriangle, q.triangleCount, q.material, q.matchMaterial) == (7, 5, 3, 6, -1, 1)
    assert R.bake_params(7, 5, triangles=(2, 4)).triangleCount == 4
    assert R.lib().rtHipTune(b"bake_texels", 1000.0) == 0  # (a known key)
    R.tune("reset", 0)


def test_null_arguments_are_refused_without_a_device():
    L = R.lib()
    p = R.bake_params(4, 4)
    ao = np.zeros(16, F32)
    tri = np.zeros(16, np.uint32)
    assert L.rtHipSceneBakeAmbientOcclusion(None, C.byref(p), ao.ctypes.data_as(C.c_void_p), tri.ctypes.data_as(C.c_void_p)) == -1
    assert "null" in R.last_error()
    assert L.rtHipSceneBakeAmbientOcclusionDevice(None, C.byref(p), ao.ctypes.data_as(C.c_void_p), None, None) == -1
    assert "null" in R.last_error()
    with pytest.raises(ValueError):
        R.bake_params(-1, 4)
    with pytest.raises(ValueError):
        R.bake_params(4, 4, seed=1 << 32)
    with pytest.raises(ValueError):
        R.bake_params(4, 4, triangles=range(0, 10, 2))


def test_a_unit_quad_covers_every_texel_and_its_shared_edge_goes_to_the_smaller_id():
    sc = quad(8, 8)
    cu, cv = B.centres(8, 8)
    both, _, _ = B.cover(sc.tri_uv.reshape(-1, 3, 2), np.tile(cu, 8), np.repeat(cv, 8))
    win = B.coverage(sc, 8, 8)
    assert (both.sum(0) >= 1).all() and (win != NONE).all()
    on_edge = both.all(0)
    x, y = np.arange(64) % 8, np.arange(64) // 8
    assert np.array_equal(on_edge, x + y == 7)  # centres (x + 0.5) / 8 on u + v = 1: both triangles' tests pass
    assert (win[on_edge] == 0).all()
    assert np.array_equal(win, np.where(x + y <= 7, 0, 1).astype(np.uint32))
    assert np.array_equal(B.coverage(sc, 8, 8, rects=True), win)
    for W, H in ((7, 5), (1, 1), (64, 48)):  # every size: one winner per texel, the rectangle path agrees
        w = B.coverage(sc, W, H)
        assert (w != NONE).all() and np.array_equal(B.coverage(sc, W, H, rects=True), w)


def test_degenerate_and_nan_uvs_cover_nothing():
    sc = quad(8, 8)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    cases = [[(0.2, 0.2), (0.2, 0.2), (0.8, 0.9)],      # two equal corners: den = 0
             [(0.1, 0.1), (0.5, 0.5), (0.9, 0.9)],      # collinear: den = 0
             [(0.0, 0.0), (nan, 0.0), (0.0, 1.0)],
             [(nan, nan), (1.0, 0.0), (0.0, 1.0)],
             [(0.0, 0.0), (1.0, 0.0), (0.0, nan)]]
    for uv in cases:
        covered, _, _ = B.cover(np.asarray([uv], F32), *(np.repeat(c, 1) for c in (np.linspace(0.01, 0.99, 50, dtype=F32),) * 2))
        assert not covered.any(), uv
        with_uv(sc, uv + [(0, 0), (0, 0), (0, 0)])
        assert (B.coverage(sc, 16, 16) == NONE).all(), uv
        assert (B.coverage(sc, 16, 16, rects=True) == NONE).all(), uv
    with_uv(sc, [(0, 0), (inf, 0), (0, 1), (0, 0), (0, 0), (0, 0)])  # an infinite UV has an answer too (here: nothing)
    assert np.array_equal(B.coverage(sc, 16, 16), B.coverage(sc, 16, 16, rects=True))


def test_a_lone_triangle_bakes_all_one():
    sc = mesh_scene(16, 16, [(-1.0, -1.0, 3.0), (1.0, -1.0, 3.0), (0.0, 1.0, 3.0)], [(0, 1, 2)], "bake_lone")
    with_uv(sc, [(0.1, 0.1), (0.9, 0.2), (0.3, 0.8)])
    out = B.bake(sc, 16, 12, rays=8, seed=3, dilate_passes=0, with_rays=True)
    cov = out["triangle"] != NONE
    assert 0.2 < cov.mean() < 0.8
    assert len(out["texel"]) == 8 * cov.sum()
    assert (out["ao"][cov] == 1).all() and (out["ao"][~cov] == 0).all()
    full = B.bake(sc, 16, 12, rays=8, seed=3, dilate_passes=64)
    assert (full["ao"] == 1).all() and np.array_equal(full["triangle"], out["triangle"])


def test_a_closed_box_bakes_all_zero_inside_and_all_one_outside():
    sc = closed_box(inward=True)
    # (37 x 29: no texel centre lies on a UV triangle's edge, so no surface point lies on an edge of the box, where half the
    # hemisphere looks out)
    out = B.bake(sc, 37, 29, rays=8, dilate_passes=0)
    cov = out["triangle"] != NONE
    assert cov.sum() >= 12 and len(np.unique(out["triangle"][cov])) == 12
    assert (out["ao"][cov] == 0).all() and (out["ao"][~cov] == 0).all()
    short = B.bake(sc, 37, 29, rays=8, radius=1e-3, dilate_passes=0)
    assert float(short["ao"][cov].mean()) > 0.9
    outside = B.bake(closed_box(inward=False), 37, 29, rays=8, dilate_passes=0)
    assert (outside["ao"][cov] == 1).all()


def test_dilation_on_hand_made_maps():
    W = H = 5
    v = np.zeros(25, F32)
    ok = np.zeros(25, bool)
    assert (B.dilate(v, ok, W, H, 3) == 0).all()  # no valid texel: stays 0
    v[12], ok[12] = F32(0.75), True  # the centre
    assert np.array_equal(B.dilate(v, ok, W, H, 0), v)
    one = B.dilate(v, ok, W, H, 1).reshape(5, 5)
    assert (one[1:4, 1:4] == F32(0.75)).all() and one[0].sum() == 0 and one[:, 0].sum() == 0
    assert (B.dilate(v, ok, W, H, 2) == F32(0.75)).all()
    v2, ok2 = np.zeros(25, F32), np.zeros(25, bool)
    v2[0], v2[2], ok2[0], ok2[2] = F32(0.1), F32(0.7), True, True  # texel 1 sees both; texel 6 sees both (dy = -1 row)
    d = B.dilate(v2, ok2, W, H, 1)
    assert d[1] == (F32(0.1) + F32(0.7)) / F32(2) and d[6] == d[1] and d[5] == F32(0.1) and d[7] == F32(0.7) and d[8] == F32(0.7)
    assert d[0] == F32(0.1) and d[2] == F32(0.7) and d[10] == 0
    v3, ok3 = np.zeros(25, F32), np.zeros(25, bool)
    v3[[0, 1, 5]], ok3[[0, 1, 5]] = [F32(0.1), F32(0.2), F32(0.3)], True  # order: dy = -1 first, then dx: ((0.1 + 0.2) + 0.3) / 3
    assert B.dilate(v3, ok3, W, H, 1)[6] == ((F32(0.1) + F32(0.2)) + F32(0.3)) / F32(3)


def test_grid_atlas_cells_are_disjoint_and_inside_the_unit_square():
    for T, size in ((1, 16), (10, 64), (37, 128), (1000, 1024)):
        uv = S.grid_atlas_uv(T, size)
        assert uv.shape == (3 * T, 2) and uv.dtype == F32
        assert (uv > 0).all() and (uv < 1).all()
        t = uv.reshape(T, 3, 2).astype(np.float64)
        lo, hi = t.min(1), t.max(1)
        n = int(np.ceil(np.sqrt(T)))
        cell = np.stack([np.arange(T) % n, np.arange(T) // n], 1) / n
        assert (lo > cell).all() and (hi < cell + 1.0 / n).all()  # strictly inside its own cell
        e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all()
    sc = closed_box()
    win = B.coverage(sc, 32, 32)
    assert len(np.unique(win[win != NONE])) == 12
    assert S.grid_atlas_uv(0, 8).shape == (0, 2)
