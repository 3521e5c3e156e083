"""Render passes, the parts that need no GPU: the PGM / PFM sinks byte for byte, the command line's --passes, and the mesh index the
front-end records per triangle (the `mesh` pass is derived from it on the host)."""
import struct

import numpy as np

from opencl_render_amd import __main__ as cli, frontend as F


def test_pgm_sink_writes_the_high_byte_top_row_first(tmp_path):
    alpha = np.array([[0, 255, 256], [0x7FFF, 0xFF00, 0xFFFF]], np.uint16)
    path = str(tmp_path / "a.pgm")
    F.write_pgm(path, alpha)
    assert open(path, "rb").read() == b"P5\n3 2\n255\n" + bytes([0, 0, 1, 0x7F, 0xFF, 0xFF])


def test_pfm_sink_writes_little_endian_floats_bottom_row_first(tmp_path):
    depth = np.array([[1.0, 2.5], [np.inf, -0.0], [3.25, 1e-30]], np.float32)
    path = str(tmp_path / "d.pfm")
    F.write_pfm(path, depth)
    rows = [struct.pack("<2f", *depth[r].tolist()) for r in (2, 1, 0)]
    assert open(path, "rb").read() == b"Pf\n2 3\n-1.0\n" + b"".join(rows)


def test_pfm_sink_keeps_every_bit_of_the_depth(tmp_path):
    rng = np.random.default_rng(7)
    depth = rng.random((5, 7), np.float32) * 1000
    depth[1, 3] = np.inf
    path = str(tmp_path / "d.pfm")
    F.write_pfm(path, depth)
    raw = open(path, "rb").read()
    back = np.frombuffer(raw[len(b"Pf\n7 5\n-1.0\n"):], "<f4").reshape(5, 7)[::-1]
    assert raw.startswith(b"Pf\n7 5\n-1.0\n") and np.array_equal(back.view(np.uint32), depth.view(np.uint32))


def test_command_line_accepts_passes():
    args = cli.parser().parse_args(["--scene", "soup", "--passes", "out/frame"])
    assert args.passes == "out/frame"
    assert cli.parser().parse_args([]).passes is None


def test_scene_from_meshes_records_the_mesh_of_every_triangle():
    tri = F.Mesh(points=np.float32([[0, 0, 5], [1, 0, 5], [0, 1, 5]]), polygons=np.int32([[0, 1, 2, 2]]))
    quads = F.Mesh(points=np.float32([[0, 0, 6], [1, 0, 6], [1, 1, 6], [0, 1, 6]]), polygons=np.int32([[0, 1, 2, 3], [0, 1, 2, 2], [3, 2, 1, 0]]))
    sc = F.scene_from_meshes([quads, tri, quads], [dict(color=True)], [dict(type=3, dir=(0, 0, 1))], (0.3, 0.3, 0), (0.3, 0.3, 5), (0, 1, 0),
                             np.radians(40.0), 32, 24)
    assert sc.tri_mesh.dtype == np.int32
    assert sc.tri_mesh.tolist() == [0] * 5 + [1] + [2] * 5
    assert len(sc.tri_mesh) == sc.triangle_count
