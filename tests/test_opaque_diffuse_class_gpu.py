"""The opaque-diffuse logic kernel (wf_logic_kernel<.., LEAN=true>) across its whole scene class, on the GPU.

Every scenario of scenarios.CLASS (no light, one light of every type, image colours, one-texel height maps, absent and black channels,
material -1, degenerate triangles, colours on both sides of the bounce threshold) is rendered with the class kernel and with the
general one (logic_class = 0), with and without dead-shadow skipping, on watched and planned frames, and every plane must equal the
reference kernel's (tests/golden/ref_class_scenes.npz) bit for bit.  The two kernels must also send the same rays in the same rounds.
Then: the pipeline modes that change which class-kernel instantiation runs, sample batches, and the class through the drop-in layer's
scene cache, where the class has to be worked out again whenever only the materials or only the lights change."""
import copy
import os

import numpy as np
import pytest

import oracle_lib as O
import scenarios as SC
from conftest import GOLDEN
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu

CLASS_NAMES = [f.__name__ for f in SC.CLASS]
# (logic_class, dead_shadow): the default, the default without dead-shadow skipping, the general kernel, and the general kernel without it
SETTINGS = [(1, 1), (1, 0), (0, 1), (0, 0)]


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (and the product has no CPU fallback)")


@pytest.fixture(scope="module")
def stored():
    z = np.load(os.path.join(GOLDEN, "ref_class_scenes.npz"))
    return {k: z[k] for k in z.files}


def _assert_planes(got, want, what):
    for ch, g, w in zip("RGB", got, want):
        g = np.asarray(g).reshape(np.asarray(w).shape)
        bad = int((g != w).sum())
        assert bad == 0, f"{what}: plane {ch} differs in {bad}/{g.size} pixels, max |d|={int(np.abs(g.astype(int) - w.astype(int)).max())}"


def _class_scene(name, stored):
    sc = SC.class_by_name(name)()
    R.build_lists(sc)
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE, f"{name} drifted out of the opaque-diffuse class"
    return sc, [stored[f"{name}_{c}"] for c in "rgb"]


def _frames(monkeypatch, sc, env, frames=2):
    """Planes and rays per round of `frames` consecutive frames of one resident scene (the first watched, the others planned), built
    under the RT_* variables in `env`, and the path class the scene runs."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    rs = R.ResidentScene(sc, 0)
    try:
        planes, rays = [], []
        for _ in range(frames):
            rs.render()
            rs.sync()
            assert not rs.finish()
            planes.append([p.copy() for p in rs.readback()])
            rays.append(rs.round_rays(8))
        return planes, rays, rs.path_class()
    finally:
        rs.close()
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_class_kernel_general_kernel_and_reference_agree(monkeypatch, name, stored):
    sc, want = _class_scene(name, stored)
    rays = {}
    for logic_class, dead_shadow in SETTINGS:
        what = f"{name}, logic_class={logic_class}, dead_shadow={dead_shadow}"
        planes, rays[logic_class, dead_shadow], pc = _frames(monkeypatch, sc, {"RT_WF_LOGIC_CLASS": logic_class, "RT_WF_DEAD_SHADOW": dead_shadow})
        assert pc == (R.PATH_CLASS_OPAQUE_DIFFUSE if logic_class else R.PATH_CLASS_GENERAL), what
        for frame, kind in zip(planes, ("watched", "planned")):
            _assert_planes(frame, want, f"{what}, {kind} frame vs the reference")
    for dead_shadow in (0, 1):
        # the class kernel performs the general machine's operations in order and drops only branches that cannot be taken: the same
        # rays leave in the same rounds, on the watched and on the planned frame
        assert rays[1, dead_shadow] == rays[0, dead_shadow], f"{name}, dead_shadow={dead_shadow}: class kernel {rays[1, dead_shadow]}, general {rays[0, dead_shadow]}"
        assert rays[1, dead_shadow][0] == rays[1, dead_shadow][1], f"{name}: watched and planned frames trace different rays"
    assert rays[1, 1][0][0] == rays[1, 0][0][0] > 0  # the same paths start either way


# Pipeline modes that change what the class kernel runs: <FIRST, ORDERED> = <true, true> (round 0 ordered), <true, false>,
# <false, true> (later ordered rounds), <false, false>, look-ahead off, rays cut into many short segments, every batch watched.
PIPELINE_MODES = [
    {"RT_WF_LOOKAHEAD": "0"},
    {"RT_WF_APPEND_RAYS": "0"},
    {"RT_WF_APPEND_RAYS": "4000000000", "RT_WF_ORDERED_FIRST": "0"},
    {"RT_WF_SEG": "8,8,8,8,8", "RT_WF_SEG_RAYS": "1,1,1,1"},
    {"RT_WF_BLOCKING": "1"},
]


@pytest.mark.parametrize("env", PIPELINE_MODES, ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("name", ["class_textured_bumped", "class_light_type_8", "class_degenerate_outside"])
def test_class_kernel_under_pipeline_modes(monkeypatch, name, env, stored):
    sc, want = _class_scene(name, stored)
    planes, _, pc = _frames(monkeypatch, sc, env)
    assert pc == R.PATH_CLASS_OPAQUE_DIFFUSE
    for frame, kind in zip(planes, ("watched", "planned")):
        _assert_planes(frame, want, f"{name} with {env}, {kind} frame vs the reference")


def test_class_sample_batches_accumulate_in_order(monkeypatch):
    """S=5 and a positional light, with a path-state budget that fits about 1 and about 2 samples per batch of the one tile."""
    sc = S.make_soup(80, 60, 2000, 0.12, seed=91, samples=5, random_uv=True,
                     materials=[SC._lambert(), SC._lambert(color=SC._img(92, 5, 3), bump=(40, 200, 7))],
                     lights=[dict(type=S.LIGHT_SPOT, pos=(0.1, 0.0, 2.9), col=(0.9, 0.8, 1.2), radius=0.2, half_att=1.5)])
    R.build_lists(sc)
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE
    want = O.oracle_render(sc, threads=os.cpu_count() or 1)
    for mb in ("20", "40"):
        planes, _, pc = _frames(monkeypatch, sc, {"RT_WF_STATE_MB": mb})
        assert pc == R.PATH_CLASS_OPAQUE_DIFFUSE
        for frame, kind in zip(planes, ("watched", "planned")):
            _assert_planes(frame, want, f"state budget {mb} MB, {kind} frame")


def _channel_texel(sc, material, channel):
    """Index in the atlas of a one-texel channel."""
    i = S.CH_COUNT * material + channel
    assert tuple(sc.mat_size[i]) == (1, 1)
    return int(sc.mat_start[i])


def _cache_chain():
    """A class scene of 3 x 2 tiles, then edits that take it out of the class and back in by changing only the materials or only the
    lights: (what, scene, its path class)."""
    mats = [dict(color=(255, 255, 255), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(90, 30, 200), luminance=(0, 0, 0)),
            dict(color=SC._img(81, 4, 3), reflection=(0, 0, 0), transparency=None, bump=None, luminance=(0, 0, 0))]
    light = dict(type=S.LIGHT_TUBE, pos=(0.1, 0.0, 2.8), col=(1.0, 0.9, 0.8), radius=0.1, half_att=1.5)
    base = S.make_soup(300, 200, 6000, 0.06, seed=81, samples=2, materials=mats, lights=[light], random_uv=True)
    R.build_lists(base)
    chain = [("class scene", base, R.PATH_CLASS_OPAQUE_DIFFUSE)]

    refl = _channel_texel(base, 0, S.CH_REFLECTION)
    shiny = copy.copy(base)  # only the atlas changes: sizes and starts stay
    shiny.textures = base.textures.copy()
    shiny.textures[refl, :3] = 200
    chain.append(("one reflection texel made (200,200,200)", shiny, R.PATH_CLASS_GENERAL))
    chain.append(("the reflection texel black again", base, R.PATH_CLASS_OPAQUE_DIFFUSE))

    glow = copy.copy(base)
    glow.textures = base.textures.copy()
    glow.textures[_channel_texel(base, 1, S.CH_LUMINANCE), :3] = (30, 20, 10)
    chain.append(("one luminance texel made non-black", glow, R.PATH_CLASS_GENERAL))

    bumpy = copy.copy(base)
    bumpy.mat_size, bumpy.mat_start, bumpy.textures = S.pack_materials([dict(mats[0], bump=SC._img(82, 2, 2)), mats[1]])
    chain.append(("the one-texel height map replaced by a 2x2 image", bumpy, R.PATH_CLASS_GENERAL))
    chain.append(("back to the class scene", base, R.PATH_CLASS_OPAQUE_DIFFUSE))

    two = copy.copy(base)
    two.light_type, two.light_pos, two.light_dir, two.light_col, two.light_radius, two.light_half_att = S.pack_lights(
        [light, dict(type=S.LIGHT_DISTANT, dir=(0.3, -0.8, 0.5), col=(0.5, 0.5, 0.5))])
    chain.append(("a second light", two, R.PATH_CLASS_GENERAL))
    chain.append(("the second light removed", base, R.PATH_CLASS_OPAQUE_DIFFUSE))
    return chain


@pytest.mark.parametrize("instances", [1, 3])
def test_class_follows_edits_through_the_scene_cache(monkeypatch, instances):
    """RaytraceAll keeps its last scene resident and rebuilds a part by content hash; the path class is derived per part (build_materials,
    build_lights, clone_part).  A class that were not worked out again would render a reflective or glowing scene as diffuse.  With 3
    instances the all-GPUs id deals the 6 tiles over instances 0-2, and instances 1 and 2 copy every part from instance 0."""
    threads = os.cpu_count() or 1
    n = R.lib().rtHipDeviceCount()
    R.lib().rtHipCacheClear()
    if instances > 1:
        monkeypatch.setenv("RT_HIP_VIRTUAL_DEVICES", str(instances))
    try:
        for what, sc, want_class in _cache_chain():
            assert R.path_class(sc) == want_class, what
            ok, r, g, b = R.raytrace_all(n + 1 if instances > 1 else 1, sc)
            assert ok, R.last_error()
            _assert_planes((r, g, b), O.oracle_render(sc, threads=threads), f"{instances} instance(s), {what}")
    finally:
        R.lib().rtHipCacheClear()
