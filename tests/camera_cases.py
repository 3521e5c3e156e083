"""Camera poses and list helpers shared by the camera-move tests (tests/test_camera_move.py, tests/test_camera_move_gpu.py).

The scenarios of tests/scenarios.py are soups in the frustum of a camera at the origin that looks along +z (centres 2..4 deep, so the
soup's middle is (0, 0, 3)).  POSES are rigid moves of that camera: a small pan, a quarter orbit about the vertical axis through the
soup's middle, the eye in the middle of the soup's depth range (triangles on both sides of the eye plane and across it), and the
original pose again.  The oracle for a pose is the Scene copy with the camera replaced and the lists of oracle_lib.oracle_camera_list."""
import copy

import numpy as np

import oracle_lib as O

TILE = 128
CENTRE = np.array([0.0, 0.0, 3.0])
SCENES = ("lambert_distant", "mixed_materials_textured", "mirror_hall", "all_light_types", "degenerate_and_outside", "odd_size_multi_tile")
POSES = ("pan", "orbit90", "inside", "home")
MIN_SHARE = 0.25  # of the image's pixels with a non-empty list, in at least three of the four poses


def _rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def camera_fields(sc, pose):
    """(eye, eye_to_top_left, left_to_right, top_to_bottom, pixel_size_inv) of `pose` applied to the scene's own camera: float32 rows of 4."""
    eye, tl, lr, tb = (np.asarray(v, np.float64)[:3] for v in (sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    if pose == "pan":
        eye = eye + np.array([0.15, 0.05, 0.0])
    elif pose == "orbit90":
        m = _rot_y(90.0)
        eye, tl, lr, tb = CENTRE + m @ (eye - CENTRE), m @ tl, m @ lr, m @ tb
    elif pose == "inside":
        eye = eye + np.array([0.0, 0.0, 3.0])
    elif pose == "shifted":  # (the builder families start from this one)
        eye = eye + np.array([0.07, -0.04, 0.02])
    elif pose != "home":
        raise KeyError(pose)

    def f4(v):
        out = np.zeros(4, np.float32)
        out[:3] = v
        return out
    return f4(eye), f4(tl), f4(lr), f4(tb), float(np.float32(sc.pixel_size_inv))


def posed(sc, pose, lists=True):
    """A copy of the scene seen from `pose`, with the ORACLE's camera lists for it (the grid does not depend on the camera)."""
    out = copy.copy(sc)
    out.eye, out.eye_to_top_left, out.left_to_right, out.top_to_bottom, out.pixel_size_inv = camera_fields(sc, pose)
    if lists:
        out.cam_start, out.cam_end, out.cam_list = O.oracle_camera_list(out)
    return out


def share_non_empty(sc):
    return float(np.count_nonzero(sc.cam_end > sc.cam_start)) / sc.pixels


def row_major_of(width, height, tiles):
    """For every tile-major index slot*128*128 + ly*128 + lx of the instance's tiles: the row-major pixel, or -1 outside the image."""
    tiles_x = (width + TILE - 1) // TILE
    tiles = np.asarray(tiles, np.int64)
    ly, lx = np.divmod(np.arange(TILE * TILE, dtype=np.int64), TILE)
    gx = (tiles % tiles_x)[:, None] * TILE + lx[None, :]
    gy = (tiles // tiles_x)[:, None] * TILE + ly[None, :]
    return np.where((gx < width) & (gy < height), gy * width + gx, -1).reshape(-1)


def flatten(start, end, lst):
    """(lengths, concatenated contents) of the per-pixel lists lst[start[p] .. end[p]) in the order of p."""
    start, end = start.astype(np.int64), np.maximum(end.astype(np.int64), start.astype(np.int64))
    n = end - start
    total = int(n.sum())
    if total == 0:
        return n, np.zeros(0, np.uint32)
    idx = np.repeat(start - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(total)
    return n, lst[idx]


def assert_lists_equal(rs, want, label):
    """Every tile-major pixel of the resident scene reads what the row-major lists of `want` (a Scene) give that pixel; pixels of a tile
    that lie outside the image read nothing.  Returns the entry count of the instance's pixels (before any de-duplication)."""
    start, end, lst = rs.scene_view("cam_start"), rs.scene_view("cam_end"), rs.camera_list()
    rm = row_major_of(want.width, want.height, rs.tiles)
    assert start.shape == end.shape == rm.shape, label
    assert np.all(end >= start) and (lst.size == 0 or int(end.max()) <= lst.size), f"{label}: a range leaves the list"
    inside = rm >= 0
    n_got, got = flatten(start, end, lst)
    assert not n_got[~inside].any(), f"{label}: pixels outside the image hold entries"
    ws, we = np.zeros(rm.size, np.uint32), np.zeros(rm.size, np.uint32)
    ws[inside], we[inside] = want.cam_start[rm[inside]], want.cam_end[rm[inside]]
    n_want, exp = flatten(ws, we, want.cam_list)
    bad = np.nonzero(n_got != n_want)[0]
    assert bad.size == 0, f"{label}: {bad.size} pixels differ in list length, first tile-major {bad[:5]} (got {n_got[bad[:5]]}, want {n_want[bad[:5]]})"
    assert np.array_equal(got, exp), f"{label}: list contents differ"
    return int(n_want.sum())
