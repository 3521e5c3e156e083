"""The parts of the geometry update that need no device: argument checks of the C entry points, the array marshalling of set_vertices, the
--spin command line and the spin's vertices.  (The update itself: tests/test_geometry_move_gpu.py.)  Every test here needs the symbols,
methods and options of this feature."""
import ctypes as C

import numpy as np
import pytest

from opencl_render_amd import __main__ as cli, raytrace as R


def test_null_arguments_are_refused_without_a_device():
    L = R.lib()
    up = R.GeometryUpdate()
    not_a_scene = C.c_void_p(16)  # never dereferenced: the NULL update is refused first
    for args in ((None, C.byref(up)), (not_a_scene, None)):
        L.rtHipTune(b"reset", 0.0)  # (any successful call; the error text below must be this call's)
        assert L.rtHipSceneSetGeometry(*args) == -1
        assert "null argument" in R.last_error()
    log = (C.c_uint64 * 6)()
    assert L.rtHipTestSceneGeometryLog(None, C.byref(log), 6) == -1 and "null argument" in R.last_error()
    ms = (C.c_double * 4)()
    assert L.rtHipTestSceneGeometryTimes(None, C.byref(ms)) == -1
    # cl_uint, three pointers at 8-byte alignment, cl_int, padded to the pointers' alignment
    assert C.sizeof(R.GeometryUpdate) == 40
    assert R.GeometryUpdate.vertex.offset == 8 and R.GeometryUpdate.arraysOnDevice.offset == 32


class Recorder(R.ResidentScene):
    def __init__(self, triangles):  # no device: only the marshalling runs
        self.scene = type("S", (), dict(triangle_count=triangles, vertex=None, tri_index=None, tri_normal=None))()
        self.handle = None
        self.device = 0
        self.calls = []

    def _set_geometry(self, vertex, tri_index, tri_normal, on_device):
        self.calls.append((vertex, tri_index, tri_normal, on_device))
        return 0


def test_set_vertices_pads_and_refuses():
    rs = Recorder(2)
    v3 = np.arange(15, dtype=np.float32).reshape(5, 3)
    idx3 = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    n4 = np.ones((6, 4), np.float32)
    rs.set_vertices(v3, idx3, n4)
    v, idx, nrm, dev = rs.calls[-1]
    assert not dev and v.shape == (5, 4) and v.dtype == np.float32 and v.flags.c_contiguous
    assert np.array_equal(v[:, :3], v3) and not v[:, 3].any()
    assert idx.shape == (2, 4) and idx.dtype == np.int32 and np.array_equal(idx[:, :3], idx3) and not idx[:, 3].any()
    assert nrm.shape == (6, 4) and np.array_equal(nrm, n4)
    # self.scene describes what is resident
    assert np.array_equal(rs.scene.vertex, v) and np.array_equal(rs.scene.tri_index, idx) and np.array_equal(rs.scene.tri_normal, nrm)
    rs.set_vertices(np.zeros((7, 4), np.float32))  # [V, 4] goes through as it is; index and normals stay
    v, idx, nrm, dev = rs.calls[-1]
    assert v.shape == (7, 4) and idx is None and nrm is None
    assert rs.scene.vertex.shape == (7, 4) and rs.scene.tri_index.shape == (2, 4)
    calls = len(rs.calls)
    for bad, exc in (((v3.astype(np.float64),), TypeError), ((np.zeros((5, 2), np.float32),), ValueError), ((np.zeros(15, np.float32),), ValueError),
                     ((v3, idx3.astype(np.int64)), TypeError), ((v3, np.zeros((3, 3), np.int32)), ValueError),
                     ((v3, None, np.zeros((5, 3), np.float32)), ValueError), ((v3, None, np.zeros((6, 3), np.float64)), TypeError)):
        with pytest.raises(exc):
            rs.set_vertices(*bad)
    assert len(rs.calls) == calls  # a refused update reaches nothing
    rs.__class__._set_geometry = lambda self, *a: -3
    try:
        before = rs.scene
        assert rs.try_set_vertices(v3) == -3 and rs.scene is before
        with pytest.raises(RuntimeError):
            rs.set_vertices(v3)
    finally:
        del rs.__class__._set_geometry


def test_spin_arguments_and_file_names():
    args = cli.parse_args(["--spin", "8", "--out", "dir.v2/turn.bmp", "--passes", "p/x", "--denoise", "d.pfm", "--ao", "ao.pgm"])
    assert args.spin == 8 and args.orbit == 1
    assert cli.orbit_outputs(args, 0) == dict(out="dir.v2/turn_000.bmp", passes="p/x_000", denoise="d_000.pfm", ao="ao_000.pgm")
    assert cli.orbit_outputs(args, 7)["out"] == "dir.v2/turn_007.bmp"
    assert cli.parse_args(["--out", "img.ppm"]).spin == 1
    for bad in (["--spin", "0"], ["--spin", "-2"], ["--spin", "4", "--orbit", "4"], ["--spin", "4", "--bake-ao", "b.pfm"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    assert "--spin" in cli.parser().format_help()


def test_spin_vertices():
    """Pose 0 is the input bit for bit; heights and lane 3 are copied exactly; pose N/4 of a known point is where the angle says (the turn
    is computed in fp64 and rounded to fp32 once: half an ulp of the coordinate's magnitude, bounded here by 2^-23 * 4); the sense of the
    turn is orbit_positions': the eye's quarter pose and the vertices' quarter pose of the same point agree."""
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(50, 4)).astype(np.float32) * 3
    centre = (0.25, -1.0, 3.0)
    assert R.spin_vertices(pts, centre, 0, 12).tobytes() == pts.tobytes()
    assert R.spin_vertices(pts, centre, 12, 12).tobytes() == pts.tobytes()
    for i in range(1, 12):
        out = R.spin_vertices(pts, centre, i, 12)
        assert out.dtype == np.float32 and out[:, 1].tobytes() == pts[:, 1].tobytes() and out[:, 3].tobytes() == pts[:, 3].tobytes()
        r0 = np.hypot(pts[:, 0].astype(np.float64) - centre[0], pts[:, 2].astype(np.float64) - centre[2])
        r1 = np.hypot(out[:, 0].astype(np.float64) - centre[0], out[:, 2].astype(np.float64) - centre[2])
        assert np.all(np.abs(r1 - r0) <= 4 * 2.0 ** -23 * (np.abs(centre[0]) + np.abs(centre[2]) + r0))
    quarter = R.spin_vertices(np.float32([[0.0, 2.0, -3.0]]), (0.0, 0.0, 0.0), 1, 4)
    assert np.allclose(quarter, [[-3.0, 2.0, 0.0]], atol=1e-6) and quarter[0, 1] == np.float32(2.0)
    assert np.allclose(quarter[0], R.orbit_positions((0.0, 2.0, -3.0), (0.0, 0.0, 0.0), 4)[1], atol=1e-6)
    assert np.allclose(R.spin_directions(np.float32([[1.0, 0.0, 0.0]]), 1, 4), [[0.0, 0.0, -1.0]], atol=1e-6)
    assert pts.shape == (50, 4) and R.spin_vertices(pts[:, :3], centre, 3, 12).shape == (50, 3)
