"""Scenes and change sequences shared by the motion-vector tests (tests/test_motion.py shows on the oracle alone that they are not vacuous,
tests/test_motion_gpu.py runs them on the device).

A step is (what becomes current, whether the scene is marked again BEFORE the change).  camera_steps() / geometry_steps() turn a sequence
into (label, current Scene, reference Scene, moves) tuples: the states the oracle compares.  Grids and camera lists come from the host
builders, which are not under test here."""
import dataclasses

import numpy as np

import camera_cases as CC
import geometry_cases as GC
import scenarios
from opencl_render_amd import raytrace as R

F32 = np.float32
# name -> crop.  The issue's list was camera_cases.SCENES at 24 x 16 (odd_size_multi_tile at 136 x 132), with the rule that a scene whose
# pairs fail the shares below is swapped for another of camera_cases.SCENES / scenarios.AXIS.  Measured on the oracle (central crops, hit
# share over the four camera pairs): lambert_distant 0.03..0.09, mixed_materials_textured 0.04..0.15, all_light_types 0.01..0.09,
# degenerate_and_outside 0.00..0.14, odd_size_multi_tile 0.06..0.22 -- all below MIN_HIT -- and mirror_hall 0.67..0.97.  The AXIS rooms hit
# everywhere, but in their central 24 x 16 window no point lies behind the `inside` camera; at the larger crops below some do.  So the
# soups are swapped for the two AXIS scenes that are larger than a tile, each cropped to several tiles with one partly outside the image.
CAMERA_SCENES = {"mirror_hall": (24, 16), "axis_near_axis_mixed": (136, 132), "axis_class_sun": (136, 120)}
GEOMETRY_SCENES = {"mirror_hall": (24, 16), "axis_planes_fine": (24, 16)}

# mark at "home"; the mark stays for pan and orbit90 and is renewed before inside and before home
CAMERA_SEQUENCE = (("pan", False), ("orbit90", False), ("inside", True), ("home", True))
# mark at the base shape; reindex moves no triangle; a new mark (the same shape, re-indexed); then two updates without a mark -- twist is
# measured against the base shape: a reference that aliased the update's spare set would read translate's records --, a mark, collapse
GEOMETRY_SEQUENCE = (("reindex", False), ("translate", True), ("twist", False), ("collapse", True))
MIN_HIT, MIN_MOVED = 0.20, 0.10


def crop(sc, w, h):
    """The central w x h window of sc's image (the same camera, its top-left moved to the window's), camera lists rebuilt."""
    w, h = min(w, sc.width), min(h, sc.height)
    x0, y0 = (sc.width - w) // 2, (sc.height - h) // 2
    tl = np.asarray(sc.eye_to_top_left, F32).copy()
    lr, tb = np.asarray(sc.left_to_right, F32), np.asarray(sc.top_to_bottom, F32)
    tl[:3] = (tl[:3] + lr[:3] * F32(x0)) + tb[:3] * F32(y0)
    out = dataclasses.replace(sc, width=w, height=h, eye_to_top_left=tl, cam_start=None, cam_end=None, cam_list=None)
    R.build_camera_list(out, threads=16)
    return out


_base = {}
_grid = [R.build_scene_grid]


def use_grid_builder(build):
    """build(Scene) fills box_min, grid_start, grid_list: the host builder by default; the GPU tests pass the device builder, which is
    quicker on the rooms' large triangles and makes the same grid."""
    _grid[0] = build


def base_scene(name, size):
    """Scenario `name` (of scenarios.py, AXIS included) with its grid, cropped to size (cached: the tests do not change it)."""
    if (name, size) not in _base:
        sc = scenarios.axis_by_name(name)() if name.startswith("axis_") else getattr(scenarios, name)()
        _grid[0](sc)
        _base[name, size] = crop(sc, *size)
    return _base[name, size]


def posed(sc, pose):
    """A copy of the scene seen from `pose` (no lists: the walk reads the grid only)."""
    return CC.posed(sc, pose, lists=False)


def shaped(sc, name):
    """(arrays of deformation `name` of the BASE scene sc, the Scene they make with the host builder's grid)."""
    arrays = GC.arrays(sc, name)
    out = GC.with_arrays(sc, *arrays, lists=False)
    _grid[0](out)
    return arrays, out


def camera_steps(sc, sequence=CAMERA_SEQUENCE):
    """[(pose, current Scene, reference Scene, mark before the move, moves)] for a scene marked at its own pose first."""
    steps, ref, cur_pose, ref_pose = [], sc, "home", "home"
    cur = sc
    for pose, mark in sequence:
        if mark:
            ref, ref_pose = cur, cur_pose
        cur, cur_pose = posed(sc, pose), pose
        steps.append((pose, cur, ref, mark, cur_pose != ref_pose))
    return steps


def geometry_steps(sc, sequence=GEOMETRY_SEQUENCE):
    """[(deformation, arrays, current Scene, reference Scene, mark before the update, moves)] for a scene marked at its base shape first."""
    steps, ref, cur = [], sc, sc
    for name, mark in sequence:
        if mark:
            ref = cur
        arrays, cur = shaped(sc, name)
        steps.append((name, arrays, cur, ref, mark, name != "reindex"))  # (reindex is measured against the shape it re-indexes)
    return steps


def mixed_case():
    """Camera and geometry both changed between the mark and the call: (base, arrays, current Scene, reference Scene)."""
    sc = base_scene("mirror_hall", (24, 16))
    arrays, bent = shaped(sc, "twist")
    return sc, arrays, posed(bent, "pan"), sc


def shares(out):
    """(share of the pixels that hit, share of the hit pixels whose motion is longer than a pixel, pixels with prev_t <= 0)."""
    hit = out["triangle"] != 0xFFFFFFFF
    with np.errstate(all="ignore"):
        m = out["motion"].astype(np.float64)
        far = np.sqrt(m[..., 0] ** 2 + m[..., 1] ** 2) > 1.0  # (NaN: not counted)
    return float(hit.mean()), float((far & hit).sum() / max(int(hit.sum()), 1)), int((hit & (out["prev_t"] <= 0)).sum())
