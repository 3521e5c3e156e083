"""The opaque-diffuse logic kernel (wf_logic_kernel<.., LEAN>) against the general one (tuning key logic_class = 0) and the oracle:
bit-identical planes on scenes of that class, on watched and planned frames."""
import os

import numpy as np
import pytest

import oracle_lib as O
import scenarios as SC
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (and the product has no CPU fallback)")


def _assert_planes(got, want, what):
    for ch, g, w in zip("RGB", got, want):
        g = np.asarray(g).reshape(np.asarray(w).shape)
        bad = int((g != w).sum())
        assert bad == 0, f"{what}: plane {ch} differs in {bad}/{g.size} pixels"


def _frames(monkeypatch, sc, logic_class, frames):
    """Planes of `frames` consecutive frames of one resident scene (the first watched, the others planned)."""
    monkeypatch.setenv("RT_WF_LOGIC_CLASS", str(logic_class))
    rs = R.ResidentScene(sc, 0)
    try:
        assert rs.path_class() == (R.path_class(sc) if logic_class else R.PATH_CLASS_GENERAL)
        out = []
        for _ in range(frames):
            rs.render()
            assert not rs.finish()
            out.append([p.copy() for p in rs.readback()])
        return out
    finally:
        rs.close()


@pytest.mark.parametrize("name", ["lambert_distant", "soup_640x360_s2", "lambert_1m"])
def test_opaque_diffuse_kernel_matches_general_kernel_and_oracle(monkeypatch, name):
    if name == "lambert_distant":
        sc = SC.lambert_distant()
    elif name == "soup_640x360_s2":
        sc = S.make_soup(640, 360, 60_000, 0.012, seed=77, samples=2)
    else:
        import bench
        sc = bench.make_scene("lambert_1m", 1)  # BASELINE config 3: 1920x1080, 1 M triangles (lists built)
    if name != "lambert_1m":
        R.build_lists(sc)
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE
    want = O.oracle_render(sc, threads=os.cpu_count() or 1)
    lean = _frames(monkeypatch, sc, 1, 2)
    general = _frames(monkeypatch, sc, 0, 2)
    for i, what in enumerate(("watched", "planned")):
        _assert_planes(lean[i], general[i], f"{name}, {what} frame: class kernel vs general kernel")
        _assert_planes(lean[i], want, f"{name}, {what} frame: class kernel vs oracle")


def test_general_scene_keeps_the_general_kernel(monkeypatch):
    sc = SC.mirror_hall()
    R.build_lists(sc)
    monkeypatch.setenv("RT_WF_LOGIC_CLASS", "1")
    rs = R.ResidentScene(sc, 0)
    try:
        assert rs.path_class() == R.PATH_CLASS_GENERAL
    finally:
        rs.close()
