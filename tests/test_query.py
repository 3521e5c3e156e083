"""Ray queries without a GPU: the C ABI declares and exports rtHipSceneIntersect / rtHipSceneIntersectDevice with 32- and 16-byte ray
and hit records, intersect() fails loudly where there is no device, and -- where the reference's kernel file was built -- the reference's
own RayIntersectsTriangles gives exactly what the restatement rt_oracle_grid_trace gives on every ray set (the contract the device
is checked against in test_query_gpu.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import query_cases as Q
import scenarios
from conftest import ROOT, load_golden_scene
from opencl_render_amd import raytrace as R, scene as S


def test_header_declares_the_query_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ("rtHipSceneIntersect", "rtHipSceneIntersectDevice"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert re.search(r"typedef struct rtHipRay \{ cl_float o\[3\]; cl_float tmin; cl_float d\[3\]; cl_float tmax; \} rtHipRay;", text)
    assert re.search(r"typedef struct rtHipHit \{ cl_float t; cl_uint triangle; cl_float abL; cl_float acL; \} rtHipHit;", text)
    assert C.sizeof(R.Ray) == 32 and C.sizeof(R.Hit) == 16
    assert [f[0] for f in R.Hit._fields_] == ["t", "triangle", "abL", "acL"]


def test_query_argument_errors_need_no_device(hip_lib):
    hip_lib.rtHipSceneIntersect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    hip_lib.rtHipSceneIntersectDevice.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_void_p]
    assert hip_lib.rtHipSceneIntersect(None, None, None, 0, None) == -1  # a NULL scene
    assert hip_lib.rtHipSceneIntersectDevice(None, None, None, 4, None, None) == -1


def test_intersect_fails_loudly_without_a_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() > 0:
        pytest.skip("a GPU is present: test_query_gpu.py covers the device path")
    sc = S.make_soup(64, 48, 200, 0.1, seed=4)
    R.build_lists(sc)
    # without a device no resident scene can exist (there is no CPU stand-in to query) ...
    with pytest.raises(RuntimeError, match="rtHipSceneCreate"):
        R.ResidentScene(sc)
    # ... and a query through a scene object that holds none fails loudly in the library instead of returning empty answers
    rs = R.ResidentScene.__new__(R.ResidentScene)
    rs.scene, rs.device, rs.handle = sc, 0, None
    with pytest.raises(RuntimeError, match="rtHipSceneIntersect failed: null scene"):
        rs.intersect(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))


GOLDEN_SCENES = ("mirror_hall", "degenerate_and_outside", "sparse_many_samples")
AXIS_SCENES = ("axis_planes_fine", "axis_untame_far", "axis_untame_tiny", "axis_near_axis_mixed")


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref/libref_kernel.so not built (the reference tree is absent)")
@pytest.mark.parametrize("name", GOLDEN_SCENES + AXIS_SCENES)
def test_reference_walk_equals_the_restatement_on_every_ray_set(name, tmp_path_factory):
    sc = load_golden_scene(name)[0] if name in GOLDEN_SCENES else scenarios.axis_by_name(name)()
    work = str(tmp_path_factory.mktemp("ref_shim"))
    for kind, rs in Q.all_sets(sc, n=400, seed=7).items():
        want = Q.oracle_answers(sc, rs)
        got = Q.reference_answers(sc, rs, work)
        bad = Q.mismatches(got, want, hits_only=True)
        assert bad.size == 0, f"{name}/{kind}: {bad.size} rays differ, first {bad[:5]}"
        if kind in ("camera", "segments"):
            assert (want["triangle"] != Q.NONE).any(), f"{name}/{kind}: no ray hits anything"
