"""Split logic rounds (tuning key logic_split): in the opaque-diffuse class with look-ahead on, a round >= 1 runs wf_answer_kernel (the
answers as a stream: shadow answers folded, paths with nothing left finished, paths whose bounce hit something listed) and
wf_shade_kernel (the listed paths' hits, one lane each).  Neither the planes nor the rays of any round may change: logic_split on,
logic_split off and the oracle (or the reference kernel's stored planes) agree bit for bit on a watched frame and on planned ones,
at S = 1 and S = 4 -- for dense and empty shade lists, dead shadow rays, no light, lights that leave lmin >= lmax, every pipeline mode
and frames whose sample window moves.  Scenes outside the class must not take the new launches.

lmin >= lmax: in this class lmin is 0 and lmax the distance to the light's sampled point (or infinite), so the branch is taken
exactly when the light draws no point at all (type 0 and unknown types: scenarios.CLASS holds both, every hit takes it)."""
import dataclasses
import os

import numpy as np
import pytest

import oracle_lib as O
import scenarios as SC
from conftest import GOLDEN
from opencl_render_amd import raytrace as R, scene as S
from pipeline_modes import MODES, mode_id

pytestmark = pytest.mark.gpu

THREADS = min(os.cpu_count() or 1, 16)


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (and the product has no CPU fallback)")


def _assert_planes(got, want, what):
    for ch, g, w in zip("RGB", got, want):
        g = np.asarray(g).reshape(np.asarray(w).shape)
        bad = int((g != w).sum())
        assert bad == 0, f"{what}: plane {ch} differs in {bad}/{g.size} pixels"


def _with_triangles(sc, first, pts):
    """`sc` with triangles first.. replaced by pts [n, 3, 3] (flat normals), in place."""
    pts = np.asarray(pts, np.float32)
    n = len(pts)
    sc.vertex[3 * first:3 * (first + n), :3] = pts.reshape(-1, 3)
    nrm = np.cross(pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 0]).astype(np.float32)
    nrm /= np.sqrt((nrm * nrm).sum(1, dtype=np.float32))[:, None]
    sc.tri_normal[3 * first:3 * (first + n), :3] = np.repeat(nrm, 3, axis=0)
    return sc


def _soup(samples):
    """The headline scene in small (tests/test_dead_shadow_gpu.py): about one bounce in nine hits something."""
    return S.make_soup(640, 360, 60_000, 0.012, seed=77, samples=samples)


def _backlit(samples):
    """Its back-lit twin: most shadow rays of the camera hits are dead, so the bounce is the main ray of round 1."""
    return S.make_soup(640, 360, 60_000, 0.012, seed=78, samples=samples,
                       lights=[dict(type=S.LIGHT_DISTANT, dir=(0.6, -0.3, -0.74), col=(1, 1, 1), radius=0.3)])


def _room(samples):
    """A closed box around the camera and a soup, lit by a point light inside: every bounce hits something."""
    soup = 3000
    sc = S.make_soup(200, 150, soup + 12, 0.1, seed=83, samples=samples,
                     lights=[dict(type=S.LIGHT_SPOT, pos=(0.3, 1.0, 2.0), col=(1.0, 0.9, 0.8), radius=0.1, half_att=4.0)])
    lo, hi = np.array([-4.0, -3.0, -2.0]), np.array([4.0, 3.0, 6.0])
    c = np.array([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])])
    quads = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    tris = [[c[a], c[b], c[d]] for a, b, d, e in quads] + [[c[a], c[d], c[e]] for a, b, d, e in quads]
    return _with_triangles(sc, soup, tris)


def _wall(samples):
    """One large triangle facing the camera, nothing behind it: no bounce hits anything, every shade list is empty."""
    sc = S.make_soup(200, 150, 1, 0.1, seed=84, samples=samples)
    return _with_triangles(sc, 0, [[(-10.0, -10.0, 3.0), (10.0, -10.0, 3.0), (0.0, 15.0, 3.0)]])


def _no_light(samples):
    """No light: the shade pass finishes its paths without sending a ray."""
    return S.make_soup(320, 200, 20_000, 0.03, seed=85, samples=samples, lights=[])


def _point(samples):
    """A point light inside the soup: finite shadow ranges, N.L of either sign."""
    return S.make_soup(320, 200, 20_000, 0.03, seed=86, samples=samples,
                       lights=[dict(type=S.LIGHT_SPOT, pos=(0.1, -0.05, 3.0), col=(0.9, 0.8, 0.7), radius=0.15, half_att=1.5)])


def _general(samples):
    """General path class (tests/test_dead_shadow_gpu.py): two lights and a transparent material."""
    mats = [dict(color=(255, 255, 255), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0)),
            dict(color=(230, 240, 250), reflection=(0, 0, 0), transparency=(200, 210, 220), bump=(0, 0, 0), luminance=(0, 0, 0))]
    lights = [dict(type=S.LIGHT_DISTANT, dir=(0.3, -0.8, 0.5), col=(0.8, 0.8, 0.7), radius=0.4),
              dict(type=S.LIGHT_SPOT, pos=(0.4, 0.6, 1.5), col=(0.9, 0.7, 0.6), radius=0.2, half_att=2.0)]
    return S.make_soup(256, 192, 8000, 0.05, seed=79, samples=samples, materials=mats, lights=lights)


SCENES = {"soup": _soup, "backlit": _backlit, "room": _room, "wall": _wall, "no_light": _no_light, "point": _point}
_cache = {}


def _scene(name, samples):
    """(scene with its lists built, the oracle's planes): made once per module, never written to."""
    key = (name, samples)
    if key not in _cache:
        sc = (SCENES.get(name) or _general)(samples)
        R.build_lists(sc)
        want = O.oracle_render(sc, threads=THREADS)
        for p in want:
            p.setflags(write=False)
        _cache[key] = (sc, want)
    return _cache[key]


def _frames(monkeypatch, sc, split, env=None, frames=3):
    """Planes, rays per round and (split rounds issued, shade-list lengths) of `frames` consecutive frames of one resident scene (the
    first watched, the others planned), built under logic_split = `split` and the RT_* variables in `env`; and the scene's path class."""
    env = dict(env or {}, RT_WF_LOGIC_SPLIT=str(split))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    rs = R.ResidentScene(sc, 0)
    try:
        planes, rays, shade = [], [], []
        for _ in range(frames):
            rs.render()
            rs.sync()
            assert not rs.finish()
            planes.append([p.copy() for p in rs.readback()])
            rays.append(rs.round_rays(8))
            shade.append(rs.shade_log(8))
        return planes, rays, shade, rs.path_class()
    finally:
        rs.close()
        for k in env:
            monkeypatch.delenv(k)


def _compare(monkeypatch, sc, want, what, env=None, expect_split=True):
    on, rays_on, shade_on, pc = _frames(monkeypatch, sc, 1, env)
    off, rays_off, shade_off, _ = _frames(monkeypatch, sc, 0, env)
    print(f"{what}: rays per round {rays_on[0]}, split rounds and shade lists {shade_on}")
    for i, kind in enumerate(("watched", "planned", "planned again")):
        _assert_planes(on[i], off[i], f"{what}, {kind} frame: logic_split on vs off")
        _assert_planes(on[i], want, f"{what}, {kind} frame: logic_split on vs the reference")
        assert rays_on[i] == rays_off[i], f"{what}, {kind} frame: rays per round {rays_on[i]} with the key on, {rays_off[i]} with it off"
        assert shade_off[i][0] == 0, f"{what}, {kind} frame: logic_split = 0 issued split rounds"
        assert (shade_on[i][0] > 0) == expect_split, f"{what}, {kind} frame: split rounds {shade_on[i][0]}"
    assert rays_on[0] == rays_on[1] == rays_on[2], f"{what}: watched and planned frames trace different rays"
    return rays_on[0], shade_on, pc


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_split_rounds_keep_planes_and_rays(monkeypatch, name, samples):
    sc, want = _scene(name, samples)
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE
    rays, shade, pc = _compare(monkeypatch, sc, want, f"{name}, S={samples}")
    assert pc == R.PATH_CLASS_OPAQUE_DIFFUSE
    listed = shade[0][1]  # (the watched frame launches every shade pass, so every round's list is logged)
    if name == "wall":
        assert rays[0] > 0 and sum(listed) == 0, (rays, listed)
    elif name == "room":
        assert listed[1] > 0.9 * rays[0], f"a closed room: {listed[1]} of {rays[0]} paths listed in round 1"
    else:
        assert 0 < listed[1] < rays[0], (rays, listed)
    if name == "no_light":
        assert rays[2] == 0, rays  # (no shadow ray leaves the shade pass)
    if name == "backlit":
        assert rays[1] < 1.5 * rays[0], rays  # (most camera hits sent the bounce alone)


def test_an_empty_list_skips_the_shade_launch_and_the_frame_finishes(monkeypatch):
    """The wall's planned frames launch no shade pass (their plan says 0 listed paths), log nothing and are complete."""
    sc, want = _scene("wall", 1)
    on, _, shade, _ = _frames(monkeypatch, sc, 1, frames=4)
    for i in range(4):
        _assert_planes(on[i], want, f"frame {i}")
        assert shade[i][0] > 0 and sum(shade[i][1]) == 0


def test_a_listed_path_behind_a_skipped_shade_launch_is_noticed(monkeypatch):
    """Should a planned frame skip a shade launch (forced here: every one) and the round list a path all the same, the answer kernel
    raises RT_WF_ERR_GRID and finish() renders the frame again, watched."""
    monkeypatch.setenv("RT_WF_PLAN_SHADE_SKIP", "1")
    sc, want = _scene("point", 1)
    rs = R.ResidentScene(sc, 0)
    try:
        rs.render()
        assert not rs.finish()
        _assert_planes(rs.readback(), want, "watched frame")
        rs.render()
        assert rs.finish() is True
        _assert_planes(rs.readback(), want, "frame redone after a skipped shade launch")
    finally:
        rs.close()


@pytest.mark.parametrize("samples", [1, 4])
def test_a_general_scene_takes_no_split_rounds(monkeypatch, samples):
    sc, want = _scene("general", samples)
    assert R.path_class(sc) == R.PATH_CLASS_GENERAL
    _, _, pc = _compare(monkeypatch, sc, want, f"general, S={samples}", expect_split=False)
    assert pc == R.PATH_CLASS_GENERAL


@pytest.fixture(scope="module")
def stored():
    z = np.load(os.path.join(GOLDEN, "ref_class_scenes.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", [f.__name__ for f in SC.CLASS])
def test_split_rounds_across_the_scene_class(monkeypatch, name, stored):
    sc = SC.class_by_name(name)()
    R.build_lists(sc)
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE
    _compare(monkeypatch, sc, [stored[f"{name}_{c}"] for c in "rgb"], name)


@pytest.mark.parametrize("env", MODES, ids=mode_id)
def test_split_rounds_under_pipeline_modes(monkeypatch, env):
    sc, want = _scene("soup", 1)
    _compare(monkeypatch, sc, want, f"soup under {env}", env=env, expect_split=env.get("RT_WF_LOOKAHEAD") != "0")


def test_split_rounds_follow_a_moving_sample_window(monkeypatch):
    """One sample per frame of a sequence of 4 (divisor 4, advancing): successive planned frames draw other samples, so their shade
    lists differ in length.  Every frame equals the frame a fresh, watched, unsplit scene renders for that window; the four frames of
    a cycle sum to the oracle's 4-sample frame (no add saturates, so a plain sum is the ordered one); no frame is redone."""
    sc4, want = _scene("soup", 4)
    sc = dataclasses.replace(sc4, sample_count=1)
    for k, v in {"RT_WF_BLOCKING": "1", "RT_WF_LOGIC_SPLIT": "0"}.items():
        monkeypatch.setenv(k, v)
    ref = []
    for f in range(4):
        rs = R.ResidentScene(sc, 0)
        try:
            rs.set_sample_window(4, f, 4)
            rs.render()
            ref.append([p.copy() for p in rs.readback()])
        finally:
            rs.close()
    summed = [sum(r[c].astype(np.uint32) for r in ref) for c in range(3)]
    assert max(int(s.max()) for s in summed) < 65535
    _assert_planes(summed, want, "the four windows' frames, summed, vs the oracle's 4-sample frame")
    monkeypatch.delenv("RT_WF_BLOCKING")
    monkeypatch.setenv("RT_WF_LOGIC_SPLIT", "1")
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_sample_window(4, 0, 4, advance=True)
        lists = []
        for i in range(9):  # (frames after the first are planned)
            rs.render()
            rs.sync()
            assert not rs.finish(), f"frame {i} was rendered again"
            assert rs.sample_window()["last"]["first"] == i % 4
            _assert_planes(rs.readback(), ref[i % 4], f"frame {i}: window f = {i % 4}")
            rounds, listed = rs.shade_log(4)
            assert rounds > 0
            lists.append(listed[1])
        print(f"shade list of round 1 per frame: {lists}")
        assert len(set(lists[:4])) > 1, "the windows' shade lists have the same length"
        assert lists[4:8] == lists[:4]
    finally:
        rs.close()
