"""GPU case for the file readers (run with -m gpu): generated OBJ + MTL scenes -> frontend.read_obj -> scene_from_meshes -> both lists
built on the device -> a resident scene's frame and its material-id pass.  The frame must be, bit for bit, the CPU oracle's frame of
the scene made from the INDEPENDENT reader's mesh and materials (tests/fileio_oracle.py) with lists from the host builders; one scene
also goes through the command line, its BMP compared byte for byte."""
import os

import numpy as np
import pytest

import fileio_cases as FC
import fileio_oracle as FO
import oracle_lib as O
from opencl_render_amd import frontend as F, raytrace as R, scene as S

pytestmark = pytest.mark.gpu

W, H, SAMPLES = 64, 48, 2


def _scene(mesh, materials, name):
    cam = FC.GPU_CAMERA
    return F.scene_from_meshes([mesh], materials, [dict(type=S.LIGHT_DISTANT, dir=cam["light_dir"])], cam["eye"], cam["look_at"], (0, 1, 0),
                               np.radians(cam["fov"]), W, H, samples=SAMPLES, name=name)


def test_generated_obj_scenes_render_as_the_reference_readers_scene(tmp_path, hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device (the product has no CPU fallback)")
    scenes = FC.write_gpu_scenes(str(tmp_path))
    assert len(scenes) == 3
    features = dict(unmapped=0, mixed_vn=0, fan=0, negative=0)
    for path, textured in scenes:
        ref = FO.read_obj(path)
        want_sc = _scene(F.Mesh(ref.points, ref.polygons, ref.corner_normals, ref.corner_uv, ref.polygon_material), FO.material_dicts(ref), path)
        assert 150 <= want_sc.triangle_count <= 400
        R.build_lists(want_sc)  # the host builders equal the independent builder oracle (tests/test_builders.py)
        want = O.oracle_render(want_sc, threads=min(16, os.cpu_count() or 1))
        has_vn = ref.corner_normals.reshape(len(ref.polygons), -1).any(axis=1)
        features["mixed_vn"] += bool(has_vn.any() and not has_vn.all())
        features["unmapped"] += bool((ref.polygon_material == -1).any())
        features["fan"] += any(len(line.split()) > 5 for line in open(path, "rb").read().split(b"\n") if line.startswith(b"f "))
        features["negative"] += b" -" in open(path, "rb").read()

        mesh, materials = F.read_obj(path)
        sc = _scene(mesh, materials, path)
        R.build_camera_list_device(sc, 0)
        R.build_scene_grid_device(sc, 0)
        rs = R.ResidentScene(sc, 0)
        try:
            rs.set_passes(triangle=True)
            rs.render()
            got = rs.readback()
            passes = rs.readback_passes()
        finally:
            rs.close()
        for ch, g, e in zip("RGB", got, want):
            assert np.array_equal(np.asarray(g).reshape(H, W), np.asarray(e).reshape(H, W)), f"{path}: plane {ch} differs from the oracle in {(np.asarray(g).reshape(-1) != np.asarray(e).reshape(-1)).sum()} values"
        # not a blank agreement
        hit = passes["triangle"] != 0xFFFFFFFF
        assert ((passes["material"] == -1) & hit).any(), f"{path}: no pixel shows a face without a material"
        names = [m["name"].decode() for m in ref.materials]
        for name in textured:
            assert (passes["material"][hit] == names.index(name)).any(), f"{path}: material {name} is not seen"
        r = np.asarray(want[0]).reshape(-1)
        assert (r > 0).mean() > 0.4 and (r == 65535).mean() < 0.25 and len(np.unique(r >> 8)) > 50, path
    assert all(features.values()), features
    R.lib().rtHipCacheClear()


def test_generated_obj_scene_through_the_command_line(tmp_path, hip_lib):
    from opencl_render_amd import __main__ as cli
    path, textured = FC.write_gpu_scenes(str(tmp_path))[2]
    cam = FC.GPU_CAMERA
    out = str(tmp_path / "cli.bmp")
    argv = ["--obj", path, "--eye"] + [str(v) for v in cam["eye"]] + ["--look-at"] + [str(v) for v in cam["look_at"]] + \
           ["--fov", str(cam["fov"]), "--light-dir"] + [str(v) for v in cam["light_dir"]] + \
           ["--width", str(W), "--height", str(H), "--samples", str(SAMPLES), "--out", out]
    assert cli.main(argv) == 0
    ref = FO.read_obj(path)
    sc = _scene(F.Mesh(ref.points, ref.polygons, ref.corner_normals, ref.corner_uv, ref.polygon_material), FO.material_dicts(ref), path)
    R.build_lists(sc)
    want = O.oracle_render(sc, threads=min(16, os.cpu_count() or 1))
    want_path = str(tmp_path / "oracle.bmp")
    F.write_bmp(want_path, *want)
    data = open(out, "rb").read()
    assert data == open(want_path, "rb").read() and len(data) == 54 + W * H * 3
    assert FO.read_image(out).tobytes() == F.planes_to_rgb8(*[np.asarray(p).reshape(H, W) for p in want]).tobytes()  # the independent reader reads the library's file
    R.lib().rtHipCacheClear()
