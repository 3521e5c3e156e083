"""Scenes for the list builders, shared by the host tests (tests/test_builders.py) and the device tests
(tests/test_builders_gpu.py), each a family where a builder can go wrong: soups of several sizes, degenerate and snapped
triangles, near triangles with huge projections, mesh scenes (shared vertices, few distinct coordinates, so repeated split
planes and zero-width cells), triangles behind the eye, coordinates of both zero signs, one triangle over the whole image,
one-pixel-wide images, long per-pixel lists, the camera builder's one-thread / workgroup boundary, and empty scenes.

CASES maps a name to a function that builds the scene afresh (the builders write into it).  Every scene keeps its oracle run to
a few seconds."""
import os

import numpy as np

from opencl_render_amd import demo, frontend as F, scene as S

HERE = os.path.dirname(os.path.abspath(__file__))

# The camera builder's boundary (RT_BIG_RECT in rt_build_device.hip): a triangle whose clipped rectangle has more pixels than
# this is rasterised by a workgroup, else by one thread.
BIG_RECT = 1024


def with_triangles(sc, pts):
    """sc with its geometry replaced by the triangles pts [k,3,3] (one vertex each, flat normals, no UVs)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3, 3)
    k = len(pts)
    sc.vertex = np.zeros((3 * k, 4), np.float32)
    sc.vertex[:, :3] = pts.reshape(-1, 3)
    sc.tri_index = np.zeros((k, 4), np.int32)
    sc.tri_index[:, 0] = 3 * np.arange(k)
    sc.tri_index[:, 1] = sc.tri_index[:, 0] + 1
    sc.tri_index[:, 2] = sc.tri_index[:, 0] + 2
    sc.tri_material = np.zeros(k, np.int32)
    sc.tri_uv = np.zeros((3 * k, 2), np.float32)
    n = np.cross(pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 0]).astype(np.float32)
    ln = np.sqrt((n * n).sum(1)).astype(np.float32)
    ln[ln == 0] = 1
    sc.tri_normal = np.zeros((3 * k, 4), np.float32)
    sc.tri_normal[:, :3] = np.repeat(n / ln[:, None], 3, axis=0)
    return sc


def unproject(sc, x, y, depth):
    """The point at `depth` times the eye-to-pixel vector of pixel coordinates (x, y): it projects back to (x, y)."""
    d = sc.eye_to_top_left[:3] + sc.left_to_right[:3] * np.float32(x) + sc.top_to_bottom[:3] * np.float32(y)
    return (sc.eye[:3] + np.float32(depth) * d).astype(np.float32)


def _soup_72x56():
    return S.make_soup(72, 56, 1200, 0.12, seed=77)


def _soup_200x150():
    return S.make_soup(200, 150, 2500, 0.08, seed=20)                     # several tiles, ragged edges


def _larger_than_image():
    return S.make_soup(64, 48, 300, 1.4, seed=8)                          # triangles larger than the image, many off-screen vertices


def _near():
    return S.make_soup(97, 61, 900, 0.3, seed=9, depth=(0.2, 6.0))        # near triangles: huge projections, some straddle the image border


def _degenerate():
    deg = S.make_soup(56, 40, 900, 0.12, seed=18)                         # zero-area and axis-parallel triangles
    v = deg.vertex.reshape(-1, 3, 4)
    v[::7, 1] = v[::7, 0]; v[::7, 2] = v[::7, 0]
    v[::11, 2] = v[::11, 1]
    v[::5, 1, 1] = v[::5, 0, 1]                                           # horizontal edge ab (slope division by zero, :143-150)
    v[::3, 2, 0] = v[::3, 1, 0]                                           # vertical edge bc
    return deg


def _snapped():
    snap = S.make_soup(80, 60, 600, 0.2, seed=10)                         # vertices exactly on pixel corners / split planes
    snap.vertex[:, :3] = np.round(snap.vertex[:, :3] * 16) / 16 + np.float32(0)  # (+0 turns -0.0 into +0.0: where equal keys land is the sort's business, in the reference too)
    return snap


def _signed_zeros():
    """The snapped soup with its negative zeros kept: coordinates -0.0 and +0.0 compare equal, so every sort may order them its
    own way, and a plane taken at a run of zeros may come out with either sign."""
    sc = S.make_soup(80, 60, 600, 0.2, seed=10)
    sc.vertex[:, :3] = np.round(sc.vertex[:, :3] * 16) / 16
    sc.meta["signed_zeros"] = True
    return sc


def _room():
    return demo.room_scene(200, 150)                                       # every triangle over more than 48 cells


def obj_scene(samples=1):
    """tests/data/scene.obj at the camera of test_obj_file_to_image_file_on_the_gpu."""
    mesh, materials = F.read_obj(os.path.join(HERE, "data", "scene.obj"))
    return F.scene_from_meshes([mesh], materials, [dict(type=S.LIGHT_DISTANT, dir=(0.3, -0.8, 0.5))], (2.6, 2.2, -3.4), (0, 0.4, 0), (0, 1, 0),
                               np.radians(55.0), 192, 128, samples=samples)


def _behind_the_eye():
    # triangles behind the eye and across the eye plane: the reference does not clip them (trianglelist.cpp:547, quoted in demo.py)
    return S.make_soup(96, 72, 800, 0.3, seed=31, depth=(-2.0, 3.0))


def _whole_image():
    """One triangle around the whole image: every pixel's list is [0], so the de-duplication chains are W + H - 2 long."""
    sc = S.make_soup(150, 110, 1, 0.1, seed=5)
    w, h = sc.width, sc.height
    return with_triangles(sc, [[unproject(sc, -w, -h, 3.0), unproject(sc, 3 * w, -h, 3.0), unproject(sc, -w, 3 * h, 3.0)]])


def _image_1x1():
    return S.make_soup(1, 1, 60, 0.4, seed=41)


def _image_1xn():
    return S.make_soup(1, 53, 300, 0.1, seed=42)                          # one column


def _image_nx1():
    return S.make_soup(67, 1, 300, 0.1, seed=43)                          # one row


def _stacked():
    """About 2 000 triangles over one 6 x 6 pixel patch, at shuffled depths: per-pixel lists of ~2 000 entries that the device
    fills in atomic order and must sort.  (V > 3 T: the vertex array also holds vertices no triangle uses.)"""
    sc = S.make_soup(64, 48, 1, 0.1, seed=6)
    rng = np.random.Generator(np.random.PCG64(44))
    k = 2000
    tris = []
    for _ in range(k):
        z = rng.uniform(1.5, 5.0)
        xy = rng.uniform(-3.0, 3.0, (3, 2)) + (29.0, 21.0)
        tris.append([unproject(sc, x, y, z * rng.uniform(0.95, 1.05)) for x, y in xy])
    # make sure the patch is covered by most: a third of them are large enough to hold the whole patch
    for t in range(0, k, 3):
        tris[t] = [unproject(sc, 24.0, 16.0, 2.0 + t / k), unproject(sc, 40.0, 16.0, 2.0 + t / k), unproject(sc, 24.0, 32.0, 2.0 + t / k)]
    sc = with_triangles(sc, tris)
    # The split planes are quantiles of ALL vertices: unused ones spread over the room keep the patch to a few planes per axis,
    # so that the grid (and the oracle's serial build of it) stays small.
    spread = np.zeros((150_000, 4), np.float32)
    spread[:, :3] = rng.uniform((-4.0, -3.0, 1.0), (4.0, 3.0, 6.0), (150_000, 3)).astype(np.float32)
    sc.vertex = np.concatenate([sc.vertex, spread])
    return sc


# (x0, y0, width, height): rectangles of exactly 1 024 and 1 025 pixels, in several shapes and places
BOUNDARY_RECTS = [(4, 3, 32, 32), (60, 70, 16, 64), (90, 5, 64, 16), (120, 100, 32, 32),
                  (8, 60, 41, 25), (100, 30, 25, 41), (50, 112, 41, 25), (130, 40, 25, 41)]


def _boundary():
    """Triangles whose clipped rectangle (pixels x0 .. x0 + w - 1, y0 .. y0 + h - 1) is exactly BIG_RECT pixels, and others at
    BIG_RECT + 1: the vertices are the unprojected pixel coordinates x0 + 0.5 .. x0 + w - 0.5, far from any pixel boundary."""
    sc = S.make_soup(192, 144, 1, 0.1, seed=7)
    tris = []
    for i, (x0, y0, w, h) in enumerate(BOUNDARY_RECTS):
        z = 2.0 + 0.25 * i
        a, b, c = (x0 + 0.5, y0 + 0.5), (x0 + w - 0.5, y0 + 0.5), (x0 + 0.5, y0 + h - 0.5)
        if i % 2:
            a, b, c = (x0 + w - 0.5, y0 + h - 0.5), (x0 + 0.5, y0 + h - 0.5), (x0 + w - 0.5, y0 + 0.5)  # the other half, other winding
        tris.append([unproject(sc, x, y, z) for x, y in (a, b, c)])
    sc = with_triangles(sc, tris)
    sc.meta["rect_area"] = [w * h for _, _, w, h in BOUNDARY_RECTS]
    return sc


def _no_triangles():
    sc = S.make_soup(48, 32, 10, 0.1, seed=45)
    sc.tri_index, sc.tri_material = sc.tri_index[:0].copy(), sc.tri_material[:0].copy()
    sc.tri_uv, sc.tri_normal = sc.tri_uv[:0].copy(), sc.tri_normal[:0].copy()
    return sc


def _nothing():
    sc = _no_triangles()
    sc.vertex = sc.vertex[:0].copy()
    return sc


CASES = {
    "soup_72x56": _soup_72x56,
    "soup_200x150": _soup_200x150,
    "larger_than_image": _larger_than_image,
    "near": _near,
    "degenerate": _degenerate,
    "snapped": _snapped,
    "room": _room,
    "obj": obj_scene,
    "behind_the_eye": _behind_the_eye,
    "signed_zeros": _signed_zeros,
    "whole_image": _whole_image,
    "image_1x1": _image_1x1,
    "image_1xn": _image_1xn,
    "image_nx1": _image_nx1,
    "stacked": _stacked,
    "boundary": _boundary,
    "no_triangles": _no_triangles,
    "nothing": _nothing,
}
NAMES = list(CASES)


def make(name):
    sc = CASES[name]()
    sc.name = sc.name or name
    return sc
