"""The parts of the camera move that need no device: argument checks of the C entry points, the vectors look_at hands on, the --orbit
command line and the orbit's poses.  (The move itself: tests/test_camera_move_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

from opencl_render_amd import __main__ as cli, frontend as F, raytrace as R


def test_null_arguments_are_refused_without_a_device():
    L = R.lib()
    cam = R.Camera()
    not_a_scene = C.c_void_p(16)  # never dereferenced: the NULL camera is refused first
    for call, args in ((L.rtHipSceneSetCamera, (None, C.byref(cam))), (L.rtHipSceneSetCamera, (not_a_scene, None)),
                       (L.rtHipSceneGetCamera, (None, C.byref(cam))), (L.rtHipSceneGetCamera, (not_a_scene, None))):
        L.rtHipTune(b"reset", 0.0)  # (any successful call; the error text below must be this call's)
        assert call(*args) == -1
        assert "null argument" in R.last_error()
    out = (C.c_uint64 * 3)()
    assert L.rtHipTestSceneCameraLog(None, C.byref(out)) == -1 and R.last_error()
    ptrs = (C.c_void_p * 6)()
    assert L.rtHipTestScenePointers(None, C.byref(ptrs)) == -1
    assert L.rtHipTestSceneCameraList(None, 0, 0, None) == -1
    assert C.sizeof(R.Camera) == 68  # four cl_float[4] and pixelSizeInv


POSES = [((0.0, 0.0, 0.0), (0.0, 0.0, 3.0), (0, 1, 0), 50.0, 64, 48),
         ((3.0, 1.5, -2.0), (0.25, 0.5, 1.0), (0, 1, 0), 35.0, 200, 150),
         ((-7.0, 0.1, 4.0), (1.0, -2.0, 0.5), (0.1, 1, 0), 90.0, 1920, 1080)]


@pytest.mark.parametrize("position,look_at,up,fov,w,h", POSES)
def test_look_at_hands_on_the_front_end_vectors(position, look_at, up, fov, w, h):
    class Recorder(R.ResidentScene):
        def __init__(self):  # no device: only look_at's arithmetic runs
            self.scene = type("S", (), dict(width=w, height=h))()
            self.handle = None

        def set_camera(self, *fields):
            self.fields = fields

    rs = Recorder()
    rs.look_at(position, look_at, up, np.radians(fov))
    tl, lr, tb, inv = F.set_camera(position, look_at, up, np.radians(fov), w, h)
    eye, gtl, glr, gtb, ginv = rs.fields
    assert np.asarray(eye, np.float32).tobytes() == np.asarray(position, np.float32).tobytes()
    for got, want in ((gtl, tl), (glr, lr), (gtb, tb)):
        assert np.asarray(got, np.float32).tobytes() == want.tobytes()
    assert ginv == inv and np.isfinite(inv) and np.any(lr[:3] != 0)


def test_orbit_arguments_and_file_names():
    args = cli.parse_args(["--orbit", "12", "--out", "dir.v2/turn.bmp", "--passes", "p/x", "--denoise", "d.pfm", "--ao", "ao.pgm"])
    assert args.orbit == 12
    assert cli.orbit_outputs(args, 0) == dict(out="dir.v2/turn_000.bmp", passes="p/x_000", denoise="d_000.pfm", ao="ao_000.pgm")
    assert cli.orbit_outputs(args, 11)["out"] == "dir.v2/turn_011.bmp"
    plain = cli.parse_args(["--out", "img.ppm"])
    assert plain.orbit == 1 and cli.orbit_outputs(plain, 3) == dict(out="img_003.ppm", passes=None, denoise=None, ao=None)
    assert R.orbit_path("img.bmp", 1234) == "img_1234.bmp"
    for bad in (["--orbit", "0"], ["--orbit", "-3"], ["--orbit", "4", "--bake-ao", "b.pfm"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    assert "oriented toward the" in cli.parser().format_help()


@pytest.mark.parametrize("position,look_at", [((0.0, 0.0, 0.0), (0.0, 0.0, 3.0)), ((3.0, 1.5, -2.0), (0.25, 0.5, 1.0)),
                                              ((-700.0, 0.1, 400.0), (1000.0, -2.0, 0.5))])
def test_orbit_poses_keep_height_and_distance(position, look_at):
    """Pose i is the first eye turned by i * 360 / N degrees about the vertical axis through the look-at point.  In exact arithmetic the
    turn keeps the distance to the axis r; raytrace.orbit_positions works in fp64 (errors of a few 2^-53, negligible here) and the
    camera receives the coordinates rounded to fp32: each of x and z moves by at most half an ulp, 2^-24 of its magnitude, and that
    magnitude is at most m = max(|cx|, |cz|) + r (the axis' offset plus the circle).  The distance to the axis therefore changes by at most
    sqrt(2) * 2^-24 * m for the pose and as much again for the first eye it is compared with: the bound below is 4 * 2^-24 * m, four
    half-ulps of fp32 at the coordinates' magnitude.  The height is copied, so it is equal as a float."""
    n = 72
    p0, c = np.asarray(position, np.float64), np.asarray(look_at, np.float64)
    poses = R.orbit_positions(position, look_at, n)
    assert len(poses) == n and np.array_equal(poses[0], p0)
    r = np.hypot(p0[0] - c[0], p0[2] - c[2])
    bound = 4.0 * 2.0 ** -24 * (max(abs(c[0]), abs(c[2])) + r)
    r0 = np.hypot(*(np.float64(np.float32(p0[[0, 2]])) - c[[0, 2]]))
    for i, p in enumerate(poses):
        q = np.float32(p).astype(np.float64)  # what the camera receives
        assert q[1] == np.float64(np.float32(p0[1]))
        assert abs(np.hypot(q[0] - c[0], q[2] - c[2]) - r0) <= bound, (i, p)
        want = 2 * np.pi * i / n  # and the pose is where the angle says
        got = np.arctan2(p0[0] - c[0], p0[2] - c[2]) + want
        assert np.allclose([p[0] - c[0], p[2] - c[2]], [r * np.sin(got), r * np.cos(got)], rtol=0, atol=1e-9 * max(r, 1.0))
    quarter = R.orbit_positions((0.0, 2.0, -3.0), (0.0, 0.0, 0.0), 4)[1]
    assert np.allclose(quarter, [-3.0, 2.0, 0.0], atol=1e-12)
