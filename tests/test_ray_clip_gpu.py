"""The ray clip (tuning key ray_clip, csrc/rt_ray_clip.h): grid rays without a far end stop where they leave a convex bound of the grid's
occupied cells instead of at the grid's wall.  The planes must not change -- ray_clip on, off and the oracle agree bit for bit on watched
and planned frames, with every ray cut into short segments, with look-ahead off, in both logic kernels -- the kept planes must hold every
corner of every occupied cell (also after geometry moves, and in a clone), a scene that reaches all eight corners of its box keeps none,
and on a frustum soup's and a general scene's frames the planned cell visits of every ordered round fall."""
import os

import numpy as np
import pytest

import oracle_lib as O
from clip_checks import assert_bound as _assert_bound, occupied_cells as _occupied_cells
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


def _soup(samples=1):
    """make_soup's default shape in small: a view frustum full of triangles inside an axis-aligned box it fits badly."""
    return S.make_soup(128, 128, 10_000, 0.02, seed=91, samples=samples)


def _backlit(samples=1):
    return S.make_soup(128, 128, 10_000, 0.02, seed=92, samples=samples,
                       lights=[dict(type=S.LIGHT_DISTANT, dir=(0.6, -0.3, -0.74), col=(1, 1, 1), radius=0.3)])


def _general(samples=1):
    """General path class: two lights (one with a finite range: rays with a far end, never clipped) and a transparent material."""
    mats = [dict(color=(255, 255, 255), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0)),
            dict(color=(230, 240, 250), reflection=(0, 0, 0), transparency=(200, 210, 220), bump=(0, 0, 0), luminance=(0, 0, 0))]
    lights = [dict(type=S.LIGHT_DISTANT, dir=(0.3, -0.8, 0.5), col=(0.8, 0.8, 0.7), radius=0.4),
              dict(type=S.LIGHT_SPOT, pos=(0.4, 0.6, 1.5), col=(0.9, 0.7, 0.6), radius=0.2, half_att=2.0)]
    return S.make_soup(128, 128, 6000, 0.05, seed=93, samples=samples, materials=mats, lights=lights)


def _corner_soup():
    """The frustum soup with its first eight triangles moved into the eight corners of a box around it: the occupied cells' hull is the
    grid's box, so no half-space that holds them cuts anything off."""
    sc = _soup()
    corners = [(a, b, c) for a in (-2.3, 2.3) for b in (-2.3, 2.3) for c in (1.8, 4.2)]
    for i, (a, b, c) in enumerate(corners):
        sx, sy, sz = (-1 if a > 0 else 1), (-1 if b > 0 else 1), (-1 if c > 3 else 1)
        sc.vertex[3 * i + 0, :3] = (a, b, c)
        sc.vertex[3 * i + 1, :3] = (a + sx * 0.01, b, c)
        sc.vertex[3 * i + 2, :3] = (a, b + sy * 0.01, c + sz * 0.01)
    return sc


SCENES = {"soup": _soup, "backlit": _backlit, "general": _general}
_cache = {}


def _scene_and_oracle(name, samples):
    """(scene with its lists, the oracle's planes), made once per module."""
    key = (name, samples)
    if key not in _cache:
        sc = SCENES[name](samples)
        R.build_lists(sc)
        _cache[key] = (sc, O.oracle_render(sc, threads=min(os.cpu_count() or 1, 16)))
    return _cache[key]


def _frames(monkeypatch, sc, env, frames=2, like=None):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    rs = R.ResidentScene(sc, 0, like=like)
    try:
        planes = []
        for _ in range(frames):
            rs.render()
            rs.sync()
            assert not rs.finish()
            planes.append([p.copy() for p in rs.readback()])
        assert rs.clip_applied() == (len(rs.clip_planes()) if int(env.get("RT_WF_RAY_CLIP", 1)) else 0), "the count the planning kernels read"
        return planes, rs.clip_planes()
    finally:
        rs.close()


# every ray cut at 8 visits by the logic kernels' planning tail, by the trace kernel's planner lanes (tests/test_parity_gpu.py), and look-ahead off
VARIANTS = {
    "default": {},
    "cut_logic": {"RT_WF_SEG": "8,8,8,8,8", "RT_WF_SEG_RAYS": "1,1,1,1", "RT_WF_APPEND_RAYS": "0", "RT_WF_EXTRA_FACTOR": "6"},
    "cut_trace": {"RT_WF_SEG": "8,8,8,8,8", "RT_WF_SEG_RAYS": "1,1,1,1", "RT_WF_APPEND_RAYS": "4000000000", "RT_WF_ORDERED_FIRST": "0", "RT_WF_GROUP_RAYS": "128"},
    "no_lookahead": {"RT_WF_LOOKAHEAD": "0"},
}


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_ray_clip_keeps_the_planes(monkeypatch, name, samples):
    sc, want = _scene_and_oracle(name, samples)
    assert R.path_class(sc) == (R.PATH_CLASS_GENERAL if name == "general" else R.PATH_CLASS_OPAQUE_DIFFUSE)
    on, kept = _frames(monkeypatch, sc, {"RT_WF_RAY_CLIP": 1})
    off, kept_off = _frames(monkeypatch, sc, {"RT_WF_RAY_CLIP": 0})
    assert len(kept) >= 1, "the frustum soup keeps a plane: the clip is in effect"
    assert np.array_equal(kept, kept_off), "the bound does not depend on the key"
    for i, what in enumerate(("watched", "planned")):
        _assert_planes(on[i], off[i], f"{name}, S={samples}, {what} frame: ray_clip on vs off")
        _assert_planes(on[i], want, f"{name}, S={samples}, {what} frame: ray_clip on vs oracle")


@pytest.mark.parametrize("variant", ["cut_logic", "cut_trace", "no_lookahead"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_ray_clip_keeps_the_planes_cut_and_without_look_ahead(monkeypatch, name, variant):
    sc, want = _scene_and_oracle(name, 1)
    for clip in (1, 0):
        got, kept = _frames(monkeypatch, sc, dict(VARIANTS[variant], RT_WF_RAY_CLIP=clip))
        assert len(kept) >= 1
        for i, what in enumerate(("watched", "planned")):
            _assert_planes(got[i], want, f"{name}, {variant}, ray_clip={clip}, {what} frame vs oracle")


# ---- the bound ---------------------------------------------------------------------------------------------------------------------

def test_the_bound_holds_the_occupied_cells():
    sc, _ = _scene_and_oracle("soup", 1)
    rs = R.ResidentScene(sc, 0)
    try:
        kept, share = _assert_bound(rs, sc.box_min, "frustum soup")
        print(f"frustum soup: {len(kept)} planes kept, {share:.3f} of the cell lattice cut off")
        assert 1 <= len(kept) <= 8
        assert share > 0.05
        assert rs.clip_applied() == len(kept)
    finally:
        rs.close()


def test_a_scene_that_reaches_its_box_corners_keeps_no_plane():
    sc = _corner_soup()
    R.build_lists(sc)
    rs = R.ResidentScene(sc, 0)
    try:
        cells = _occupied_cells(rs)
        have = {tuple(c) for c in cells[((cells == 0) | (cells == 255)).all(1)]}
        assert len(have) == 8, "the input: all eight corner cells are occupied"
        assert rs.clip_planes().shape == (0, 4) and rs.clip_applied() == 0
        rs.render()
        rs.sync()
        assert not rs.finish()
        _assert_planes(rs.readback(), O.oracle_render(sc, threads=min(os.cpu_count() or 1, 16)), "corner soup vs oracle")
    finally:
        rs.close()


# ---- geometry moves and clones -------------------------------------------------------------------------------------------------------

def _moved(sc, scale):
    """The soup's shape scaled about the frustum's middle in x and y: wider or narrower than the box it was uploaded with."""
    out = _soup()
    out.vertex[:, 0] = sc.vertex[:, 0] * np.float32(scale)
    out.vertex[:, 1] = sc.vertex[:, 1] * np.float32(scale)
    return out


def test_geometry_moves_and_a_clone_rebuild_the_bound():
    base, _ = _scene_and_oracle("soup", 1)
    rs = R.ResidentScene(base, 0)
    try:
        first = True
        for scale in (1.6, 0.55):  # widen, then shrink
            want = _moved(base, scale)
            R.build_lists(want)
            rs.set_vertices(want.vertex, want.tri_index if first else None)
            first = False
            kept, share = _assert_bound(rs, want.box_min, f"after the move x{scale}")
            fresh = R.ResidentScene(want, 0)
            try:
                assert np.array_equal(fresh.clip_planes(), kept.astype(np.float32)), f"x{scale}: the moved scene and a fresh upload keep different planes"
                assert len(kept) >= 1 and share > 0.05
                frames = []
                for r in (rs, fresh):
                    r.render()
                    r.sync()
                    assert not r.finish()
                    frames.append([p.copy() for p in r.readback()])
                _assert_planes(frames[0], frames[1], f"x{scale}: moved scene vs fresh upload")
                clone = R.ResidentScene(want, 0, like=rs)
                try:
                    assert np.array_equal(clone.clip_planes(), rs.clip_planes()) and clone.clip_applied() == rs.clip_applied() == len(kept)
                    clone.render()
                    clone.sync()
                    assert not clone.finish()
                    _assert_planes(clone.readback(), frames[1], f"x{scale}: clone of the moved scene vs fresh upload")
                finally:
                    clone.close()
            finally:
                fresh.close()
    finally:
        rs.close()


# ---- the clip engages ----------------------------------------------------------------------------------------------------------------

def _logged_frames(monkeypatch, sc, env):
    """Per frame (watched, planned) of a scene built with the visit log on: (rays per round, what each trace round held)."""
    for k, v in dict(env, RT_WF_VISIT_LOG=1).items():
        monkeypatch.setenv(k, str(v))
    rs = R.ResidentScene(sc, 0)
    try:
        out = []
        for _ in range(2):
            rs.render()
            rs.sync()
            assert not rs.finish()
            out.append((rs.round_rays(4), rs.round_visits(4)))
        return out
    finally:
        rs.close()


KINDS = ("shadow", "main", "bounce")
UNCUT = {"RT_WF_SEG": "4096,4096,4096,4096,4096"}
# which planning call site writes the entries of the rounds a case looks at: round 1 is planned by the round-0 logic kernel (class or
# general), a later round -- ordered only with append_rays 0 -- by wf_shade_kernel<true> (class, split rounds) or the general logic kernel
ENGAGE = {
    "soup_uncut": ("soup", dict(UNCUT, RT_WF_APPEND_RAYS="0"), (1, 2)),
    "soup_cut_as_planned": ("soup", {}, (1,)),
    "general_uncut": ("general", dict(UNCUT, RT_WF_APPEND_RAYS="0"), (1, 2)),
}


@pytest.mark.parametrize("case", sorted(ENGAGE))
def test_the_clip_lowers_the_planned_visits_of_a_frame(monkeypatch, case):
    """The frame's own entries, read back round by round: with ray_clip 1 every ordered round that has rays plans strictly fewer cell
    visits than with ray_clip 0, for the same rays with the same answers."""
    name, env, rounds = ENGAGE[case]
    sc, _ = _scene_and_oracle(name, 1)
    on = _logged_frames(monkeypatch, sc, dict(env, RT_WF_RAY_CLIP=1))
    off = _logged_frames(monkeypatch, sc, dict(env, RT_WF_RAY_CLIP=0))
    for frame, what in enumerate(("watched", "planned")):
        (rays_on, log_on), (rays_off, log_off) = on[frame], off[frame]
        assert rays_on == rays_off, (case, what)
        for r in rounds:
            a, b = log_on[r], log_off[r]
            label = f"{case}, {what} frame, round {r}"
            print(f"{label}: planned visits {b['visits']} -> {a['visits']}, entries {b['entries']} -> {a['entries']}, with an end cell "
                  f"{b['ended']} -> {a['ended']}; " + ", ".join(f"{k} {a[k]['rays']} rays {a[k]['hits']} hits" for k in KINDS))
            assert a["ordered"] == 1 and b["ordered"] == 1, label
            assert sum(a[k]["rays"] for k in KINDS) == rays_on[r] > 0, label
            for k in KINDS:
                assert (a[k]["rays"], a[k]["hits"]) == (b[k]["rays"], b[k]["hits"]), f"{label}: the {k} rays and their answers do not depend on the key"
                assert a[k]["visits"] <= b[k]["visits"], f"{label}, {k} rays"
            assert a["visits"] < b["visits"], f"{label}: the clip does not engage"
            if "RT_WF_SEG" in env and name == "soup":  # no ray is cut and none has a far end: only the clip gives an entry an end cell
                assert a["entries"] == b["entries"] == rays_on[r], label
                assert b["ended"] == 0 and a["ended"] > 0, label
