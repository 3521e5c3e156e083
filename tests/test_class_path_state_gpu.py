"""Where the opaque-diffuse class keeps its path state (csrc/rt_path_state.h: the ring allocation addressed as a plane of camera directions
and one bounce record per path; the shadow ray's far end travelling in outc.w), on the GPU.

The scene is made for what can go wrong with addresses: a 200 x 136 image (two by two tiles, both partial) whose every pixel hits a wall
of small triangles, so that paths fill every shard from index 0 to its last entry and path ids reach their largest values; a checkerboard
of small squares stands in front of the wall, whose backs the wall's bounces hit (one path in seven; the CPU oracle's counters are asserted).  The one light is positional
with a finite half-attenuation distance -- a point light (a small sphere) between the two layers, or a spot light on the camera's side --
so the far end of a shadow ray differs from path to path and feeds the falloff: a stale or zero value changes pixels.  Every frame, watched
and planned, with the class kernels and with the general ones, must equal the CPU oracle bit for bit: at S=1, at S=3 in two sample
batches (another capacity; path ids run over samples), with the split rounds, the look-ahead and the dead-shadow skip switched off (the
single class kernel reads the far end too, and the bounce becomes the main ray), and across edits that take one resident scene out of
the class and back, which switch the ring's layout between frames."""
import copy
import os

import numpy as np
import pytest

import oracle_lib as O
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT = 200, 136
THREADS = os.cpu_count() or 1
LIGHTS = {
    # between the layers: lights the wall (its shadow rays pass the squares' edges) and the squares' backs, which only bounces see
    "point": dict(type=S.LIGHT_AREA, pos=(0.15, 0.1, 2.45), col=(1.0, 0.9, 0.8), radius=0.02, half_att=0.6),
    # on the camera's side: lights both layers' fronts, the squares shadow the wall
    "spot": dict(type=S.LIGHT_SPOT, pos=(-0.3, 0.2, 0.4), col=(0.9, 1.0, 1.1), radius=0.2, half_att=1.5),
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (and the product has no CPU fallback)")


def _squares(z, x0, x1, y0, y1, step, keep):
    """Two triangles per kept cell of a step x step lattice on the plane z: [T, 3, 3] points."""
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


def wall_scene(light, samples=1):
    """The camera of make_soup (eye at the origin, looking along +z, the view 1 wide at z = 1) in front of a closed wall at z = 2.6 that
    overlaps the view on every side, and a checkerboard of squares at z = 2.3."""
    mats = [dict(color=(255, 255, 255), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0)),
            dict(color=(250, 180, 90), reflection=(0, 0, 0), transparency=None, bump=None, luminance=(0, 0, 0))]
    pts = np.concatenate([_squares(2.6, -1.4, 1.4, -1.0, 1.0, 0.1, lambda i, j: True),
                          _squares(2.3, -1.2, 1.2, -0.9, 0.9, 0.1, lambda i, j: (i + j) % 2 == 0)])
    t = len(pts)
    sc = S.make_soup(WIDTH, HEIGHT, t, 0.1, seed=7, samples=samples, materials=mats, lights=[light], name=f"wall_{light['type']}_s{samples}")
    sc.vertex[:, :3] = pts.reshape(-1, 3)
    n = np.cross(pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 0]).astype(np.float32)
    n /= np.sqrt((n * n).sum(1, dtype=np.float32))[:, None]
    sc.tri_normal[:, :3] = np.repeat(n, 3, axis=0)
    sc.tri_material[:] = (np.arange(t) // 2) % 2
    R.build_lists(sc)
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE
    return sc


def coverage(sc):
    """(primary hits, bounce hits) of the CPU oracle: with every colour black no bounce is spawned and every shaded hit is a camera hit."""
    dark = copy.copy(sc)
    dark.textures = np.zeros_like(sc.textures)
    primary = O.oracle_render(dark, threads=THREADS, with_stats=True)[1]["shadedHits"]
    return primary, O.oracle_render(sc, threads=THREADS, with_stats=True)[1]["shadedHits"] - primary


_walls = {}


def _wall(kind, samples):
    """The scene, its oracle planes -- made once per (light, samples), shared and left unchanged."""
    if (kind, samples) not in _walls:
        sc = wall_scene(LIGHTS[kind], samples)
        primary, bounce = coverage(sc)
        assert primary == WIDTH * HEIGHT * samples, f"{sc.name}: {primary} camera hits for {WIDTH * HEIGHT * samples} samples"
        assert bounce * 10 > primary, f"{sc.name}: only {bounce} bounce hits"  # (the headline scene's rounds list one path in nine)
        _walls[kind, samples] = (sc, O.oracle_render(sc, threads=THREADS))
    return _walls[kind, samples]


def _assert_planes(got, want, what):
    for ch, g, w in zip("RGB", got, want):
        g = np.asarray(g).reshape(np.asarray(w).shape)
        bad = int((g != w).sum())
        assert bad == 0, f"{what}: plane {ch} differs in {bad}/{g.size} pixels, max |d|={int(np.abs(g.astype(int) - w.astype(int)).max())}"


def _frames(monkeypatch, sc, env, frames=2):
    """Planes and rays per round of consecutive frames of one resident scene (the first watched, the others planned) built under `env`."""
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


def _class_and_general(monkeypatch, sc, want, env, what):
    rays = {}
    for logic_class in (1, 0):
        planes, rays[logic_class], pc = _frames(monkeypatch, sc, dict(env, RT_WF_LOGIC_CLASS=logic_class))
        assert pc == (R.PATH_CLASS_OPAQUE_DIFFUSE if logic_class else R.PATH_CLASS_GENERAL)
        for frame, kind in zip(planes, ("watched", "planned")):
            _assert_planes(frame, want, f"{what}, logic_class={logic_class}, {kind} frame vs the oracle")
    assert rays[1] == rays[0], f"{what}: class kernels sent {rays[1]}, general kernels {rays[0]}"
    return rays[1]


@pytest.mark.parametrize("kind", sorted(LIGHTS))
def test_every_pixel_a_path(monkeypatch, kind):
    sc, want = _wall(kind, 1)
    rays = _class_and_general(monkeypatch, sc, want, {}, f"wall, {kind} light")
    assert rays[0][0] == rays[1][0] == WIDTH * HEIGHT  # every pixel became a path: the shards are full up to their last entry
    # the squares' backs face the point light: the bounce hits send shadow rays in round 2, whose far ends the shade pass stored.  (They
    # face away from the spot light: those shadow rays are dead, and round 2 exists only with RT_WF_DEAD_SHADOW=0, test_further_modes.)
    assert (rays[0][2] > 0) == (kind == "point")


@pytest.mark.parametrize("kind", sorted(LIGHTS))
def test_three_samples_in_two_batches(monkeypatch, kind):
    """300 MB of path state hold two of the three samples of the four tiles (122 MB per sample): batches of two and of one."""
    sc, want = _wall(kind, 3)
    _class_and_general(monkeypatch, sc, want, {"RT_WF_STATE_MB": 300}, f"wall at S=3 in two batches, {kind} light")


MODES = [{"RT_WF_LOGIC_SPLIT": 0}, {"RT_WF_LOOKAHEAD": 0}, {"RT_WF_DEAD_SHADOW": 0}]


@pytest.mark.parametrize("env", MODES, ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("kind", sorted(LIGHTS))
def test_further_modes(monkeypatch, kind, env):
    sc, want = _wall(kind, 1)
    _class_and_general(monkeypatch, sc, want, env, f"wall with {env}, {kind} light")


def test_layout_switch_on_one_resident_scene():
    """RaytraceAll keeps its last scene resident and rebuilds the materials by content hash: one reflection texel made non-black takes
    the scene out of the class (the ring is addressed [capacity][12][3] again, and mirror rays fill more of its slots), black again
    brings it back.  Nothing of one layout's frame may show in the next."""
    base, want = _wall("point", 1)
    i = S.CH_COUNT * 0 + S.CH_REFLECTION
    assert tuple(base.mat_size[i]) == (1, 1)
    shiny = copy.copy(base)
    shiny.textures = base.textures.copy()
    shiny.textures[int(base.mat_start[i]), :3] = 200
    assert R.path_class(shiny) == R.PATH_CLASS_GENERAL
    R.lib().rtHipCacheClear()
    try:
        for what, sc, exp in (("class scene", base, want), ("one reflection texel made (200,200,200)", shiny, O.oracle_render(shiny, threads=THREADS)),
                              ("the reflection texel black again", base, want), ("the same scene once more", base, want)):
            ok, r, g, b = R.raytrace_all(1, sc)
            assert ok, R.last_error()
            _assert_planes((r, g, b), exp, what)
    finally:
        R.lib().rtHipCacheClear()
