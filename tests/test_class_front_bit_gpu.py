"""`front` of a parked hit in the opaque-diffuse class (csrc/rt_wf_logic_body.h, wf_answer_kernel): a class path parks behind its shadow
ray with the face entry 0.1 always, so the class kernels keep no face entry in HBM and carry `front` in bit 16 of the path's flags word.

Two small scenes (64 x 48, a few hundred triangles) of the wall of tests/test_class_path_state_gpu.py -- a closed wall that fills the
view, a checkerboard of squares in front of it whose backs the wall's bounces hit -- with an area light BETWEEN the two layers:
  front-lit   every corner normal points at the camera.  The camera hits are front facing with the light in front of the normal (front
              true, live shadow rays out of round 0); the bounce hits strike the squares' backs, against their normals, with the light on
              that back side (front false, live shadow rays out of the shade pass or the single class kernel);
  back-lit    the same triangles with every normal reversed: the camera hits are lit on the side the normal points away from (front
              false, live shadow rays out of round 0), the bounce hits are front facing.
A `front` that is lost or misread selects the other face entry in light_accum -- the light's contribution vanishes, or lands where the
reference has none -- so the planes differ from the CPU oracle's.  That the bit is exercised is asserted on the host: the signs that make
`front` from the scene's own arrays, the oracle's counters for the bounce hits, and the oracle's planes with the light put out (the light
reaches the frame only through the face entry `front` selects).

Class kernels against the general machine (logic_class 0) against the CPU oracle, watched and planned frames, with the dead-shadow skip,
the split rounds and the look-ahead each on and off, at S=1 and at S=3 in two sample batches."""
import copy
import itertools
import os

import numpy as np
import pytest

import oracle_lib as O
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT = 64, 48
THREADS = min(os.cpu_count() or 1, 16)
LIGHT = dict(type=S.LIGHT_AREA, pos=(0.15, 0.1, 2.45), col=(1.0, 0.9, 0.8), radius=0.02, half_att=0.6)
WALL_Z, SQUARES_Z = 2.6, 2.3
STATE_MB = 75  # one tile's path state is 30.5 MB per sample: two of three samples fit, batches of two and of one


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (and the product has no CPU fallback)")


def _squares(z, x0, x1, y0, y1, step, keep):
    tris = []
    nx, ny = int(round((x1 - x0) / step)), int(round((y1 - y0) / step))
    for j in range(ny):
        for i in range(nx):
            if not keep(i, j):
                continue
            ax, ay, bx, by = x0 + i * step, y0 + j * step, x0 + (i + 1) * step, y0 + (j + 1) * step
            tris.append([(ax, ay, z), (bx, ay, z), (bx, by, z)])
            tris.append([(ax, ay, z), (bx, by, z), (ax, by, z)])
    return np.array(tris, np.float32)


def wall_scene(kind, samples):
    """make_soup's camera (eye at the origin, looking along +z, the view 1 wide at z = 1); every normal is (0, 0, -1) in the front-lit
    scene and (0, 0, 1) in the back-lit one."""
    mats = [dict(color=(255, 255, 255), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0)),
            dict(color=(250, 180, 90), reflection=(0, 0, 0), transparency=None, bump=None, luminance=(0, 0, 0))]
    pts = np.concatenate([_squares(WALL_Z, -1.4, 1.4, -1.0, 1.0, 0.2, lambda i, j: True),
                          _squares(SQUARES_Z, -1.2, 1.2, -0.9, 0.9, 0.2, lambda i, j: (i + j) % 2 == 0)])
    t = len(pts)
    assert 200 <= t <= 600
    sc = S.make_soup(WIDTH, HEIGHT, t, 0.1, seed=7, samples=samples, materials=mats, lights=[LIGHT], name=f"{kind}_wall_s{samples}")
    sc.vertex[:, :3] = pts.reshape(-1, 3)
    sc.tri_normal[:, :3] = np.array((0.0, 0.0, -1.0 if kind == "front" else 1.0), np.float32)
    sc.tri_material[:] = (np.arange(t) // 2) % 2
    R.build_lists(sc)
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE
    return sc


def assert_front_is_exercised(sc, kind, samples, want):
    """From the scene's arrays and the oracle alone."""
    nz = -1.0 if kind == "front" else 1.0
    pts = sc.vertex[:, :3].reshape(-1, 3, 3)
    wall = pts[:, 0, 2] == np.float32(WALL_Z)
    light = np.array(LIGHT["pos"], np.float64)
    reach = LIGHT["radius"]
    assert SQUARES_Z + reach < light[2] < WALL_Z - reach  # every point of the light lies between the layers
    # camera rays run towards +z and hit the wall or a square's front: front = (n.d <= 0) = (nz < 0); the light is on the camera's side of
    # the wall (n.toL = nz * (light.z - WALL_Z), the sign of -nz) and behind the squares' fronts (dead or live, the same in both scenes)
    camera_front = nz < 0
    wall_ndl_nonneg = nz * (light[2] - WALL_Z) >= 0
    assert wall_ndl_nonneg == camera_front  # the wall's shadow rays are live, with front = camera_front
    # bounces leave the wall towards -z (the side of the camera hit) and strike the squares' backs: front = (n.d <= 0) = (nz > 0); the light
    # is on that back side (n.toL = nz * (light.z - SQUARES_Z), the sign of nz)
    bounce_front = nz > 0
    squares_ndl_nonneg = nz * (light[2] - SQUARES_Z) >= 0
    assert squares_ndl_nonneg == bounce_front  # the bounce hits' shadow rays are live, with front = bounce_front
    assert camera_front != bounce_front and wall.any() and (~wall).any()  # each scene parks hits with front true AND with front false
    # the oracle's counters: every sample's camera ray hits, and bounces hit the squares
    dark = copy.copy(sc)
    dark.textures = np.zeros_like(sc.textures)
    primary = O.oracle_render(dark, threads=THREADS, with_stats=True)[1]["shadedHits"]
    planes, stats = O.oracle_render(sc, threads=THREADS, with_stats=True)
    bounce = stats["shadedHits"] - primary
    assert primary == WIDTH * HEIGHT * samples, f"{sc.name}: {primary} camera hits"
    assert bounce * 20 > primary, f"{sc.name}: only {bounce} bounce hits"
    assert stats["gridRays"] >= primary + bounce  # a shadow ray per shaded hit at least (the oracle skips none)
    # ... and the light reaches most pixels, through the face entry `front` selects
    unlit = copy.copy(sc)
    unlit.light_col = np.zeros_like(sc.light_col)
    off = O.oracle_render(unlit, threads=THREADS)
    changed = np.mean([np.mean(np.asarray(a) != np.asarray(b)) for a, b in zip(want, off)])
    print(f"{sc.name}: {primary} camera hits, {bounce} bounce hits, the light changes {changed:.3f} of the plane values")
    # (the wall shows through the open half of the checkerboard and is lit all over; the squares' fronts are not)
    assert changed > 0.4, f"{sc.name}: the light changes {changed:.3f} of the plane values only"


_walls = {}


def _wall(kind, samples):
    """The scene and its oracle planes, made once per (kind, samples), shared and left unchanged."""
    if (kind, samples) not in _walls:
        sc = wall_scene(kind, samples)
        want = O.oracle_render(sc, threads=THREADS)
        assert_front_is_exercised(sc, kind, samples, want)
        _walls[kind, samples] = (sc, want)
    return _walls[kind, samples]


def _assert_planes(got, want, what):
    for ch, g, w in zip("RGB", got, want):
        g = np.asarray(g).reshape(np.asarray(w).shape)
        bad = int((g != w).sum())
        assert bad == 0, f"{what}: plane {ch} differs in {bad}/{g.size} pixels, max |d|={int(np.abs(g.astype(int) - w.astype(int)).max())}"


def _frames(monkeypatch, sc, env):
    """Planes and rays per round of a watched and a planned frame of one resident scene built under `env`."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    rs = R.ResidentScene(sc, 0)
    try:
        planes, rays = [], []
        for _ in range(2):
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


@pytest.mark.parametrize("dead_shadow,logic_split", list(itertools.product((1, 0), (1, 0))))
@pytest.mark.parametrize("kind", ["front", "back"])
def test_front_survives_the_park(monkeypatch, kind, dead_shadow, logic_split):
    for samples, lookahead in itertools.product((1, 3), (1, 0)):
        sc, want = _wall(kind, samples)
        env = {"RT_WF_DEAD_SHADOW": dead_shadow, "RT_WF_LOGIC_SPLIT": logic_split, "RT_WF_LOOKAHEAD": lookahead}
        if samples == 3:
            env["RT_WF_STATE_MB"] = STATE_MB
        what = f"{kind}-lit wall, S={samples}, {env}"
        rays = {}
        for logic_class in (1, 0):
            planes, rays[logic_class], pc = _frames(monkeypatch, sc, dict(env, RT_WF_LOGIC_CLASS=logic_class))
            assert pc == (R.PATH_CLASS_OPAQUE_DIFFUSE if logic_class else R.PATH_CLASS_GENERAL)
            for frame, stage in zip(planes, ("watched", "planned")):
                _assert_planes(frame, want, f"{what}, logic_class={logic_class}, {stage} frame vs the oracle")
        assert rays[1] == rays[0], f"{what}: class kernels sent {rays[1]}, general kernels {rays[0]}"
        # both kinds of hit park behind live shadow rays: the camera hits' in round 1, the bounce hits' in a later round
        last = rays[1][0]
        assert last[1] >= last[0] > 0 and sum(last[2:]) > 0, f"{what}: rays per round {last}"
