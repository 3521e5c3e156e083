"""Deformations shared by the geometry-update tests (tests/test_geometry_move.py, tests/test_geometry_move_gpu.py).

The scenarios of tests/scenarios.py are soups around (0, 0, 3) (camera_cases.CENTRE) seen from the origin.  A deformation maps a Scene to the
arrays an update hands over, (vertex, tri_index or None, tri_normal or None); deformed() gives the ORACLE's view of the result: a copy of
the Scene with the arrays replaced, the grid of oracle_lib.oracle_scene_grid and the camera lists of oracle_lib.oracle_camera_list.  The
oracle is never the code under test."""
import copy

import numpy as np

import oracle_lib as O
from camera_cases import CENTRE

# every deformation the issue names; "home" hands the original arrays back
NAMES = ("translate", "twist", "scale", "collapse", "reindex", "normals")
SEQUENCE = NAMES + ("home",)
MIN_CHANGED = 0.01  # of the pixels, in the oracle's planes, for every deformation but the re-indexing


def _selected_vertices(sc):
    """The vertices of one mesh: of mesh 0 where the scene knows its meshes, else of the first half of the triangles."""
    tri = np.arange(sc.triangle_count)
    mesh = getattr(sc, "tri_mesh", None)
    pick = tri[np.asarray(mesh) == np.asarray(mesh)[0]] if mesh is not None and len(mesh) == sc.triangle_count else tri[: max(sc.triangle_count // 2, 1)]
    return np.unique(sc.tri_index[pick, :3].reshape(-1))


def arrays(sc, name):
    """(vertex [V,4] f32, tri_index [T,4] i32 or None, tri_normal [3T,4] f32 or None) of deformation `name` of scene `sc`."""
    v = sc.vertex.copy()
    if name == "home":
        return v, sc.tri_index.copy(), sc.tri_normal.copy()
    if name == "translate":  # a rigid translation of one mesh
        v[_selected_vertices(sc), :3] += np.array([0.3, 0.1, -0.05], np.float32)
        return v, None, None
    if name == "twist":  # every vertex turned about the vertical axis through the soup's middle, the angle growing with the height
        p = v[:, :3].astype(np.float64) - CENTRE
        a = 0.9 * p[:, 1] + 0.35
        x, z = p[:, 0] * np.cos(a) + p[:, 2] * np.sin(a), -p[:, 0] * np.sin(a) + p[:, 2] * np.cos(a)
        v[:, 0], v[:, 2] = x + CENTRE[0], z + CENTRE[2]
        return v, None, None
    if name == "scale":  # non-uniform, about the soup's middle: every split plane of every axis moves.  With a shear term (x += 0.3 y):
        # a scale along the axes alone maps the quantile planes along with the vertices and leaves every cell's list as it was, so the
        # condition "the oracle grid's list changes" could not hold for it on any scene
        p = (v[:, :3].astype(np.float64) - CENTRE) * np.array([1.3, 0.75, 1.15])
        p[:, 0] += 0.3 * p[:, 1]
        v[:, :3] = (p + CENTRE).astype(np.float32)
        return v, None, None
    if name == "collapse":  # every tenth triangle loses its area: corner c becomes corner b (a repeated corner)
        idx = sc.tri_index.copy()
        idx[::10, 2] = idx[::10, 1]
        return v, idx, None
    if name == "reindex":  # the vertex array reversed and three copies of vertex 0 appended: V and every index change, no triangle moves
        n = sc.vertex_count
        v = np.concatenate([sc.vertex[::-1], np.repeat(sc.vertex[:1], 3, 0)]).astype(np.float32)
        idx = sc.tri_index.copy()
        idx[:, :3] = n - 1 - idx[:, :3]
        return np.ascontiguousarray(v), idx, None
    if name == "normals":  # new corner normals alone: tilted and normalised
        nrm = sc.tri_normal.copy()
        t = nrm[:, :3].astype(np.float64) + np.array([0.6, -0.45, 0.3])
        t /= np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-30)
        nrm[:, :3] = t.astype(np.float32)
        return v, None, nrm
    raise KeyError(name)


def with_arrays(sc, vertex, tri_index=None, tri_normal=None, lists=True):
    """A copy of the scene with the arrays replaced and the ORACLE's grid and camera lists for them."""
    out = copy.copy(sc)
    out.vertex = np.ascontiguousarray(vertex, np.float32)
    if tri_index is not None:
        out.tri_index = np.ascontiguousarray(tri_index, np.int32)
    if tri_normal is not None:
        out.tri_normal = np.ascontiguousarray(tri_normal, np.float32)
    if lists:
        out.box_min, out.grid_start, out.grid_list = O.oracle_scene_grid(out)
        out.cam_start, out.cam_end, out.cam_list = O.oracle_camera_list(out)
    return out


def deformed(sc, name):
    return with_arrays(sc, *arrays(sc, name))


def changed_share(planes_a, planes_b):
    """Share of the pixels in which any of the three planes differs."""
    diff = np.zeros(np.asarray(planes_a[0]).size, bool)
    for a, b in zip(planes_a, planes_b):
        diff |= np.asarray(a).reshape(-1) != np.asarray(b).reshape(-1)
    return float(diff.mean())


def grid_differs(a, b):
    return not (np.array_equal(a.grid_start, b.grid_start) and np.array_equal(a.grid_list, b.grid_list))
