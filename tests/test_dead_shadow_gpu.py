"""Dead shadow rays (tuning key dead_shadow): a light on the side of the normal whose face entry :647 does not read gets no shadow
ray.  The planes must not change: dead_shadow on, dead_shadow off and the oracle agree bit for bit, on watched and planned frames,
in the opaque-diffuse class kernel and in the general state machine.  The round log shows the rays that are no longer traced."""
import os

import numpy as np
import pytest

import oracle_lib as O
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


def _soup(samples):
    """The headline scene in small: white Lambert, the default distant light about 60 degrees from the view direction."""
    return S.make_soup(640, 360, 60_000, 0.012, seed=77, samples=samples)


def _backlit(samples):
    """The light behind the soup, about 140 degrees from the direction to the camera: most shadow rays are dead."""
    return S.make_soup(640, 360, 60_000, 0.012, seed=78, samples=samples,
                       lights=[dict(type=S.LIGHT_DISTANT, dir=(0.6, -0.3, -0.74), col=(1, 1, 1), radius=0.3)])


def _general(samples):
    """General path class: two lights (one of them a point light with a finite range) and a transparent material, so that shadow
    rays walk on through occluders (:612-626)."""
    mats = [dict(color=(255, 255, 255), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0)),
            dict(color=(230, 240, 250), reflection=(0, 0, 0), transparency=(200, 210, 220), bump=(0, 0, 0), luminance=(0, 0, 0))]
    lights = [dict(type=S.LIGHT_DISTANT, dir=(0.3, -0.8, 0.5), col=(0.8, 0.8, 0.7), radius=0.4),
              dict(type=S.LIGHT_SPOT, pos=(0.4, 0.6, 1.5), col=(0.9, 0.7, 0.6), radius=0.2, half_att=2.0)]
    return S.make_soup(256, 192, 8000, 0.05, seed=79, samples=samples, materials=mats, lights=lights)


SCENES = {"soup": _soup, "backlit": _backlit, "general": _general}


def _frames(monkeypatch, sc, dead_shadow, frames=2):
    """Planes and rays per round of `frames` consecutive frames of one resident scene (the first watched, the others planned)."""
    monkeypatch.setenv("RT_WF_DEAD_SHADOW", str(dead_shadow))
    rs = R.ResidentScene(sc, 0)
    try:
        planes, rays = [], []
        for _ in range(frames):
            rs.render()
            rs.sync()
            assert not rs.finish()
            planes.append([p.copy() for p in rs.readback()])
            rays.append(rs.round_rays(8))
        return planes, rays
    finally:
        rs.close()


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_dead_shadow_keeps_the_planes(monkeypatch, name, samples):
    sc = SCENES[name](samples)
    R.build_lists(sc)
    want_class = R.PATH_CLASS_GENERAL if name == "general" else R.PATH_CLASS_OPAQUE_DIFFUSE
    assert R.path_class(sc) == want_class
    want = O.oracle_render(sc, threads=os.cpu_count() or 1)
    on, rays_on = _frames(monkeypatch, sc, 1)
    off, rays_off = _frames(monkeypatch, sc, 0)
    for i, what in enumerate(("watched", "planned")):
        _assert_planes(on[i], off[i], f"{name}, S={samples}, {what} frame: dead_shadow on vs off")
        _assert_planes(on[i], want, f"{name}, S={samples}, {what} frame: dead_shadow on vs oracle")
    # the same paths either way; never more rays in a round with the key on
    assert rays_on[0][0] == rays_off[0][0]
    assert sum(rays_on[0][1:]) < sum(rays_off[0][1:]), (rays_on[0], rays_off[0])


def test_dead_shadow_shrinks_the_rounds(monkeypatch):
    """Headline-style soup: round 1 (camera hits' shadow rays and bounces) and round 2 (bounce hits' shadow rays) both shrink, and
    the planned frame runs the rounds the watched frame logged."""
    sc = _soup(1)
    R.build_lists(sc)
    _, on = _frames(monkeypatch, sc, 1)
    _, off = _frames(monkeypatch, sc, 0)
    print(f"rays per round, dead_shadow on: {on[0]}  off: {off[0]}")
    for frame in (on, off):
        assert frame[0] == frame[1], "watched and planned frames of the same scene trace the same rays"
    assert on[0][0] == off[0][0] > 0
    assert on[0][1] < off[0][1]
    assert on[0][2] < off[0][2]


def test_dead_shadow_can_empty_a_round(monkeypatch):
    """No bounces (colour too dark to spawn one) and the light straight behind the soup: with the key on nearly every path ends in
    round 0, and the launch plan of the planned frame follows the rounds that are left."""
    mats = [dict(color=(1, 1, 0), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0))]
    sc = S.make_soup(320, 200, 20_000, 0.02, seed=80, samples=1, materials=mats,
                     lights=[dict(type=S.LIGHT_DISTANT, dir=(0.0, 0.0, -1.0), col=(1, 1, 1), radius=0.0)])
    R.build_lists(sc)
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE
    want = O.oracle_render(sc, threads=os.cpu_count() or 1)
    on, rays_on = _frames(monkeypatch, sc, 1, frames=3)
    off, rays_off = _frames(monkeypatch, sc, 0, frames=3)
    for i in range(3):
        _assert_planes(on[i], want, f"frame {i}: dead_shadow on vs oracle")
        _assert_planes(off[i], want, f"frame {i}: dead_shadow off vs oracle")
    print(f"rays per round, dead_shadow on: {rays_on[0]}  off: {rays_off[0]}")
    assert rays_off[0][2] == 0 and rays_on[0][2] == 0  # (no bounce: nothing is left for round 2 either way)
    assert rays_on[0][1] * 4 < rays_off[0][1]
    assert rays_on[1] == rays_on[0] and rays_on[2] == rays_on[0]
