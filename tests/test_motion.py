"""Motion vectors without a GPU: the C ABI declares and exports the entry points and refuses NULL arguments; the numpy restatement
(motion_oracle.py, walks by rt_oracle_grid_trace) gives the known answers -- a camera pan over a fronto-parallel plane, a rotation over
missed pixels, no motion for the same state --, stays within a measured distance of a float64 evaluation of the same formulas, and the
(scene, change) pairs of tests/test_motion_gpu.py are not vacuous.  The device is checked against the same restatement there."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import motion_cases as MC
import motion_oracle as MO
from conftest import ROOT
from opencl_render_amd import raytrace as R
from test_ao import mesh_scene

F32 = np.float32
NONE = 0xFFFFFFFF
ENTRY_POINTS = ("rtHipSceneMotionMark", "rtHipSceneMotionReferenceCamera", "rtHipSceneMotion", "rtHipSceneMotionDevice")


def test_header_declares_the_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert "MOTION VECTORS" in text
    for method in ("mark_motion", "motion", "motion_reference_camera"):  # (the fifth entry point of the feature is the Python one)
        assert callable(getattr(R.ResidentScene, method))


def test_null_arguments_are_refused_without_a_device():
    """(An unmarked scene cannot be refused here: there is no scene without a device.  test_motion_gpu.py does it.)"""
    L = R.lib()
    out = np.full(8, -3.0, F32)
    p = out.ctypes.data_as(C.c_void_p)
    cam = R.Camera()
    assert L.rtHipSceneMotionMark(None) == -1 and "null" in R.last_error()
    assert L.rtHipSceneMotionReferenceCamera(None, C.byref(cam)) == -1 and "null" in R.last_error()
    assert L.rtHipSceneMotion(None, p, p, p, p) == -1 and "null" in R.last_error()
    assert L.rtHipSceneMotionDevice(None, p, p, p, p, None) == -1 and "null" in R.last_error()
    assert (out == -3.0).all()


# ---- known answers on the oracle alone ---------------------------------------------------------------------------------------------
DEPTH, DELTA = 3.0, 0.125


def plane_scene():
    """Two large triangles parallel to the image plane at z = DEPTH under the soup's camera (eye at the origin, looking along +z, the
    image plane at distance 1, pixel size 1 / width); they cover the image but for its top-right corner, which sees past them."""
    v = [(-2.0, -2.0, DEPTH), (2.0, -2.0, DEPTH), (2.0, 0.9, DEPTH), (-2.0, 0.9, DEPTH), (-2.0, 2.0, DEPTH), (0.6, 2.0, DEPTH), (0.6, 0.9, DEPTH)]
    return mesh_scene(48, 36, v, [(0, 1, 2), (0, 2, 3), (3, 6, 5), (3, 5, 4)], "motion_plane")


def moved(sc, eye=None, rot_y=None):
    out = copy.copy(sc)
    if eye is not None:
        out.eye = np.asarray(tuple(eye) + (0.0,), F32)
    if rot_y is not None:
        a = np.deg2rad(rot_y)
        m = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        for k in ("eye_to_top_left", "left_to_right", "top_to_bottom"):
            v = np.zeros(4, F32)
            v[:3] = m @ np.asarray(getattr(sc, k), np.float64)[:3]
            setattr(out, k, v)
    return out


def known_cases():
    """name -> (current Scene, reference Scene); each current state is traced once."""
    if not _known:
        sc = plane_scene()
        _known["pan"] = (moved(sc, eye=(DELTA, 0.0, 0.0)), sc)
        _known["rotation"] = (sc, moved(sc, rot_y=4.0))
        _known["same"] = (sc, sc)
        for name, (cur, ref) in list(_known.items()):
            out, traced = MO.motion(cur, ref, with_hits=True)
            _known[name] = (cur, ref, out, MO.project(cur, ref, traced, np.float64))
    return _known


_known = {}
# Rounding: about 30 fp32 operations lead to px, each with a relative error of 2^-24 on magnitudes up to |TL'| |w| |tb'| / den ~ 2 * W
# pixels (W = 48), and the difference px - fx cancels nothing further: 30 * 2^-24 * 96 ~ 2e-4 pixel.
ANALYTIC_TOL = 1e-3
# |fp32 - fp64| of the motion components over the three known cases, measured: 8.6e-6 pixel (the pan's hit pixels).  The bound
# is 4 x that: the arithmetic is deterministic, the factor covers other numpy / libm builds.
MEASURED_FP32_ERROR = 8.6e-6


def test_pan_over_a_fronto_parallel_plane():
    cur, ref, out, _ = known_cases()["pan"]
    hit = out["triangle"] != NONE
    assert 0.5 < hit.mean() < 1.0  # the corner misses
    want = DELTA * float(cur.pixel_size_inv) / DEPTH  # delta * pixelSizeInv / z: 2 pixels
    assert want == 2.0
    m = out["motion"][hit].astype(np.float64)
    assert np.abs(m[:, 0] - want).max() < ANALYTIC_TOL and np.abs(m[:, 1]).max() < ANALYTIC_TOL
    assert np.abs(out["t"][hit].astype(np.float64) - DEPTH).max() < 1e-5 and np.abs(out["prev_t"][hit].astype(np.float64) - DEPTH).max() < 1e-5
    # a translation does not move the background, and a miss has no depth
    assert np.abs(out["motion"][~hit]).max() < ANALYTIC_TOL
    assert np.isposinf(out["t"][~hit]).all() and np.isposinf(out["prev_t"][~hit]).all()


def test_rotation_moves_a_missed_pixel_by_the_analytic_amount():
    cur, ref, out, _ = known_cases()["rotation"]
    miss = out["triangle"] == NONE
    assert miss.sum() >= 20
    W = cur.width
    y, x = np.nonzero(miss)
    tl, lr, tb = (np.asarray(v, np.float64)[:3] for v in (cur.eye_to_top_left, cur.left_to_right, cur.top_to_bottom))
    d = tl[None, :] + lr[None, :] * (x + 0.5)[:, None] + tb[None, :] * (y + 0.5)[:, None]
    # the reference camera is the current one turned by +4 degrees about y: in its frame the direction is turned by -4 degrees
    azimuth = np.arctan2(d[:, 0], d[:, 2]) - np.deg2rad(4.0)
    horizontal = np.hypot(d[:, 0], d[:, 2])
    px = W * (np.tan(azimuth) + 0.5)                                     # TL.x = -0.5, lr.x = 1 / W, TL.z = 1
    py = W * (tl[1] - d[:, 1] / (horizontal * np.cos(azimuth)))          # TL.y = 0.5 * aspect, tb.y = -1 / W
    got = out["motion"][miss].astype(np.float64)
    assert np.abs(got[:, 0] - (px - (x + 0.5))).max() < ANALYTIC_TOL
    assert np.abs(got[:, 1] - (py - (y + 0.5))).max() < ANALYTIC_TOL
    assert np.abs(got[:, 0]).min() > 2.0  # about W * tan(4 degrees) = 3.4 pixels


def test_the_same_state_twice_does_not_move():
    cur, ref, out, _ = known_cases()["same"]
    hit = out["triangle"] != NONE
    assert np.abs(out["motion"]).max() < ANALYTIC_TOL
    assert np.abs(out["prev_t"][hit].astype(np.float64) - out["t"][hit]).max() < 1e-5


def test_fp32_stays_close_to_a_float64_evaluation_of_the_same_formulas():
    worst = 0.0
    for name, (cur, ref, out, exact) in known_cases().items():
        assert out["motion"].dtype == F32 and exact["motion"].dtype == np.float64
        assert np.array_equal(out["triangle"], exact["triangle"])
        diff = float(np.abs(out["motion"].astype(np.float64) - exact["motion"]).max())
        print(f"{name}: |fp32 - fp64| of the motion is at most {diff:.3e} pixel")
        worst = max(worst, diff)
    assert worst < 4 * MEASURED_FP32_ERROR, f"measured {worst:.3e}"


# ---- the GPU tests' pairs are not vacuous ----------------------------------------------------------------------------------------------
def check_shares(label, out, moves):
    hit, far, behind = MC.shares(out)
    print(f"{label}: hit {hit:.3f}, longer than a pixel {far:.3f} of the hits, prev_t <= 0 in {behind} pixels")
    assert hit >= MC.MIN_HIT, f"{label}: only {hit:.3f} of the crop's pixels hit"
    if moves:
        assert far >= MC.MIN_MOVED, f"{label}: only {far:.3f} of the hit pixels move by more than a pixel"
    return behind


@pytest.mark.parametrize("name", list(MC.CAMERA_SCENES))
def test_camera_pairs_are_not_vacuous(name):
    sc = MC.base_scene(name, MC.CAMERA_SCENES[name])
    behind = {}
    for pose, cur, ref, mark, moves in MC.camera_steps(sc):
        assert moves
        behind[pose] = check_shares(f"{name}/{pose}", MO.motion(cur, ref), moves)
    assert behind["home"] >= 1, f"{name}: no pixel of the home pose lies behind the `inside` camera it is measured against"


@pytest.mark.parametrize("name", list(MC.GEOMETRY_SCENES))
def test_geometry_pairs_are_not_vacuous(name):
    sc = MC.base_scene(name, MC.GEOMETRY_SCENES[name])
    for change, arrays, cur, ref, mark, moves in MC.geometry_steps(sc):
        out = MO.motion(cur, ref)
        check_shares(f"{name}/{change}", out, moves)
        if change == "reindex":  # no triangle moves: the same-state motion, bit for bit
            same = MO.motion(cur, cur)
            assert all(MO.same_bits(out[k], same[k]).all() for k in out)
            assert np.nanmax(np.abs(out["motion"])) < ANALYTIC_TOL


def test_the_mixed_pair_is_not_vacuous():
    sc, arrays, cur, ref = MC.mixed_case()
    check_shares("camera and geometry", MO.motion(cur, ref), True)
