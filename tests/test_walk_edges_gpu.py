"""The grid walk where ray directions have zero or extreme components, on the GPU (tests/test_walk_edges.py is the CPU side).

Every scene of scenarios.AXIS (radius-0 lights along each axis, hits on repeated split planes, near-axis and subnormal components,
planes outside the tame range, point lights on planes and outside the box, mirrors and glass, one opaque-diffuse class scene) is
rendered on watched and planned frames, under the pipeline modes, with the megakernel, with and without the class kernel and
dead-shadow skipping, and from device-built lists; every plane must equal the reference kernel's (tests/golden/ref_axis_scenes.npz)
bit for bit.  The walk reproduces the reference's -0.0 and NaN-head behaviour in wf_trace_kernel, in plan_ray / segments_of and in
the megakernel's walk separately, so each of them is run here.  Random axis rooms (scenarios.axis_fuzz_scene) are checked against
the live oracle."""
import copy
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import pipeline_modes as PM
import scenarios as SC
from conftest import GOLDEN
from opencl_render_amd import raytrace as R
from test_builders_gpu import assert_device_equals_oracle, device_lists

pytestmark = pytest.mark.gpu

AXIS_NAMES = [f.__name__ for f in SC.AXIS]
# the oracle's threads: a GPU box's os.cpu_count() is many times what one command may use
THREADS = min(os.cpu_count() or 1, 16)
# scenes for the pipeline modes and the per-key runs: zeros of both signs, near-axis components beside ordinary lights over several
# tiles, finite shadow rays, untame planes, bounce and see-through rays
MODE_SCENES = ["axis_suns_type_4", "axis_near_axis_mixed", "axis_point_lights", "axis_untame_far", "axis_mirror_glass"]
FUZZ_SEEDS = range(100, 112)


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (and the product has no CPU fallback)")


@pytest.fixture(scope="module")
def stored():
    z = np.load(os.path.join(GOLDEN, "ref_axis_scenes.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def axis_scene(name):
    return SC.axis_by_name(name)()


def _assert_planes(got, want, what):
    for ch, g, w in zip("RGB", got, want):
        g = np.asarray(g).reshape(np.asarray(w).shape)
        bad = int((g != w).sum())
        assert bad == 0, f"{what}: plane {ch} differs in {bad}/{g.size} pixels, max |d|={int(np.abs(g.astype(int) - w.astype(int)).max())}"


def _want(name, stored):
    return [stored[f"{name}_{c}"] for c in "rgb"]


def _frames(monkeypatch, sc, env, pipeline=None, frames=2):
    """Planes of `frames` consecutive frames of one resident scene (the first watched, the others planned) under the RT_* variables in
    `env`, and the scene's path class."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    rs = R.ResidentScene(sc, 0)
    try:
        if pipeline is not None:
            rs.set_pipeline(pipeline)
        planes = []
        for _ in range(frames):
            rs.render()
            rs.sync()
            assert not rs.finish()
            planes.append([p.copy() for p in rs.readback()])
        return planes, rs.path_class()
    finally:
        rs.close()
        for k in env:
            monkeypatch.delenv(k)


def _assert_frames(planes, want, what):
    for frame, kind in zip(planes, ("watched", "planned", "third")):
        _assert_planes(frame, want, f"{what}, {kind} frame vs the reference")


@pytest.mark.parametrize("name", AXIS_NAMES)
def test_axis_scene_matches_the_reference(monkeypatch, name, stored):
    planes, _ = _frames(monkeypatch, axis_scene(name), {})
    _assert_frames(planes, _want(name, stored), name)


@pytest.mark.parametrize("env", PM.MODES, ids=PM.mode_id)
def test_axis_scenes_under_pipeline_modes(monkeypatch, env, stored):
    for name in MODE_SCENES:
        planes, _ = _frames(monkeypatch, axis_scene(name), env)
        _assert_frames(planes, _want(name, stored), f"{name} with {env}")


@pytest.mark.parametrize("name", AXIS_NAMES)
def test_axis_scene_megakernel(monkeypatch, name, stored):
    planes, _ = _frames(monkeypatch, axis_scene(name), {}, pipeline=R.PIPELINE_MEGAKERNEL)
    _assert_frames(planes, _want(name, stored), f"{name} (megakernel)")


@pytest.mark.parametrize("logic_class", [0, 1])
@pytest.mark.parametrize("dead_shadow", [0, 1])
def test_axis_class_scene_both_logic_kernels(monkeypatch, logic_class, dead_shadow, stored):
    planes, pc = _frames(monkeypatch, axis_scene("axis_class_sun"), {"RT_WF_LOGIC_CLASS": logic_class, "RT_WF_DEAD_SHADOW": dead_shadow})
    assert pc == (R.PATH_CLASS_OPAQUE_DIFFUSE if logic_class else R.PATH_CLASS_GENERAL)
    _assert_frames(planes, _want("axis_class_sun", stored), f"axis_class_sun, logic_class={logic_class}, dead_shadow={dead_shadow}")


@pytest.mark.parametrize("dead_shadow", [0, 1])
@pytest.mark.parametrize("name", MODE_SCENES)
def test_axis_scenes_with_and_without_dead_shadow(monkeypatch, name, dead_shadow, stored):
    planes, _ = _frames(monkeypatch, axis_scene(name), {"RT_WF_DEAD_SHADOW": dead_shadow})
    _assert_frames(planes, _want(name, stored), f"{name}, dead_shadow={dead_shadow}")


@pytest.mark.parametrize("name", AXIS_NAMES)
def test_device_builders_on_axis_scenes(name, stored):
    """The device list builders against the oracle builders on rooms of repeated planes (the front-end writes no -0.0 coordinates, so
    the planes must agree byte for byte), then a frame from the device-built lists against the reference."""
    sc = axis_scene(name)
    R.tune("reset", 0)
    dev, _ = device_lists(copy.copy(sc))
    assert_device_equals_oracle(dev, O.oracle_camera_list(sc), O.oracle_scene_grid(sc), name)
    _assert_planes(R.render_resident(dev, 0), _want(name, stored), f"{name} from device-built lists")


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_axis_fuzz_scene_matches_the_oracle(monkeypatch, seed):
    sc = SC.axis_fuzz_scene(seed)
    want = O.oracle_render(sc, threads=THREADS)
    planes, _ = _frames(monkeypatch, sc, {})
    _assert_frames(planes, want, SC.axis_fuzz_summary(sc))
