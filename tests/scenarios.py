"""Seeded parity scenarios shared by the golden-fixture generator, the oracle tests and the GPU parity tests.

Each scenario is small enough for the single-thread oracle to finish in well under a second and is aimed at one
part of the reference kernel (raytrace_opencl.c line ranges in the comments).  Inputs are deterministic functions
of the seed (numpy PCG64); the golden fixtures nevertheless store the inputs themselves (tests/golden/*.npz).
"""
from __future__ import annotations

import numpy as np

from opencl_render_amd import raytrace as R, scene as S


def _tex(seed, side, lo=0, hi=256):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(lo, hi, (side, side, 3)).astype(np.uint8)


def _lambert(**kw):
    m = dict(color=(255, 255, 255), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0))
    m.update(kw)
    return m


def lambert_distant():
    """SURVEY 8d config 3 in miniature: white Lambert, one distant light, shadow ray + diffuse bounce (:589-606,:664-683)."""
    return S.make_soup(64, 48, 1500, 0.06, seed=11, samples=2, name="lambert_distant")


def primary_only():
    """luminance-only material with a texture, no lights => no secondary rays (:514-528,:639-641)."""
    return S.make_soup(96, 64, 3000, 0.05, seed=12, samples=1, materials=[S.primary_only_material(16)], lights=[],
                       random_uv=True, name="primary_only")


def all_light_types():
    """One light of every type 0..9 plus an unknown type (:566-607): sphere sampling, omni's zero contribution."""
    lights = []
    rng = np.random.Generator(np.random.PCG64(5))
    for t in list(range(10)) + [42]:
        lights.append(dict(type=t, pos=tuple(rng.uniform(-1, 1, 3) + np.array([0, 0, 1.0])), dir=tuple(rng.uniform(-1, 1, 3)),
                           col=tuple(rng.uniform(0.1, 0.6, 3)), radius=float(rng.uniform(0.05, 0.6))))
    return S.make_soup(48, 48, 1200, 0.08, seed=13, samples=1, lights=lights, name="all_light_types")


def spot_finite_range():
    """Positional lights: finite shadow-ray range => end-cell logic of the DDA (:356-362,:380-381), finite half
    attenuation => pow(0.5, d/h) (:631)."""
    lights = [dict(type=S.LIGHT_SPOT, pos=(0.4, 0.6, 1.5), col=(0.9, 0.8, 0.7), radius=0.2, half_att=2.0),
              dict(type=S.LIGHT_AREA, pos=(-0.8, -0.3, 2.5), col=(0.3, 0.5, 0.9), radius=0.05, half_att=0.75)]
    return S.make_soup(64, 40, 2000, 0.07, seed=14, samples=2, lights=lights, name="spot_finite_range")


def no_material():
    """materialId -1 (:231,:550: zero texture => black, no bounces, no bump) on half of the triangles, mixed with a lit
    textured material on the others: black pixels where a -1 triangle is nearest, and -1 triangles still occlude
    (shadow rays :612-626 treat them as opaque, bounce rays stop on them)."""
    mats = [_lambert(color=_tex(21, 6, 60, 256), bump=_tex(22, 5))]
    sc = S.make_soup(40, 40, 500, 0.3, seed=15, samples=2, materials=mats, random_uv=True, name="no_material")
    rng = np.random.Generator(np.random.PCG64(15))
    sc.tri_material[rng.random(sc.triangle_count) < 0.5] = -1
    return sc


def mixed_materials_textured():
    """Five materials with images on every channel, wrapping UVs (positive_modf :25-28), material -1 mixed in,
    smooth (un-normalised Phong) normals (:221-229), bump maps (:231-261)."""
    mats = [
        _lambert(color=_tex(1, 8)),
        _lambert(color=_tex(2, 5), bump=_tex(3, 7)),
        _lambert(color=(200, 180, 160), luminance=_tex(4, 4, 0, 90)),
        _lambert(color=_tex(5, 6), reflection=_tex(6, 3, 0, 128)),
        _lambert(color=(255, 255, 255), transparency=_tex(7, 4, 100, 256), bump=_tex(8, 9)),
    ]
    sc = S.make_soup(64, 64, 1800, 0.09, seed=16, samples=2, materials=mats, random_uv=True, smooth_normals=True,
                     lights=[dict(type=S.LIGHT_DISTANT, dir=(0.2, -0.7, 0.6), col=(0.9, 0.9, 0.8)),
                             dict(type=S.LIGHT_TUBE, pos=(0.5, 0.5, 0.5), col=(0.4, 0.3, 0.2), radius=0.1)],
                     name="mixed_materials_textured")
    rng = np.random.Generator(np.random.PCG64(99))
    sc.tri_material[rng.random(sc.triangle_count) < 0.1] = -1
    return sc


def mirror_hall():
    """Highly reflective + transparent big triangles: mirror recursion to depth 12, see-through continuation rays
    that stay 'fromCamera' (:707-722), ring-full checks (:682,:704,:721), transparent shadow chains (:609-626)."""
    mats = [
        _lambert(color=(255, 255, 255), reflection=(230, 230, 230)),
        _lambert(color=(255, 250, 245), transparency=(200, 210, 220)),
        _lambert(color=(255, 255, 255), reflection=(120, 120, 120), transparency=(120, 120, 120)),
        _lambert(color=(240, 240, 240)),
    ]
    return S.make_soup(48, 36, 300, 0.9, seed=17, samples=2, materials=mats,
                       lights=[dict(type=S.LIGHT_DISTANT, dir=(0.1, -0.9, 0.3), col=(1, 1, 1)),
                               dict(type=S.LIGHT_PHOTOMETRIC, pos=(0, 0.5, 3.0), col=(0.5, 0.5, 0.6), radius=0.3)],
                       name="mirror_hall")


def degenerate_and_outside():
    """Zero-area triangles (NaN barycentrics), a camera placed outside the scene's bounding box so secondary rays
    start outside / leave the grid (BindInCube early returns :265-322), a light with negative colour and one bright
    enough to saturate (:726-741)."""
    sc = S.make_soup(56, 40, 900, 0.12, seed=18, samples=3,
                     lights=[dict(type=S.LIGHT_DISTANT, dir=(-0.5, -0.5, 0.2), col=(3.0, 2.0, 40.0)),
                             dict(type=S.LIGHT_PARALLEL, dir=(0.5, 0.1, -0.4), col=(-0.5, 0.2, 0.1))],
                     name="degenerate_and_outside")
    # collapse every 7th triangle to a point and every 11th to a segment
    v = sc.vertex.reshape(-1, 3, 4)
    v[::7, 1] = v[::7, 0]
    v[::7, 2] = v[::7, 0]
    v[::11, 2] = v[::11, 1]
    return sc


def sparse_many_samples():
    """Few triangles, many empty pixels and long empty DDA walks; S=5 exercises per-sample truncation (:728-740)."""
    return S.make_soup(80, 60, 150, 0.5, seed=19, samples=5, name="sparse_many_samples")


def odd_size_multi_tile():
    """Image larger than one 128x128 tile with ragged edges (tile partition)."""
    return S.make_soup(200, 150, 2500, 0.08, seed=20, samples=1, name="odd_size_multi_tile")


ALL = [lambert_distant, primary_only, all_light_types, spot_finite_range, no_material, mixed_materials_textured,
       mirror_hall, degenerate_and_outside, sparse_many_samples, odd_size_multi_tile]

FRESH_SEEDS = (101, 202, 303)


def fresh_soup(seed):
    """Random materials (every channel, bump maps), random lights of types 0..9 and a smooth-normal soup, drawn from the seed
    alone: scenes nobody picked, beside the curated ones above.  The reference's planes for FRESH_SEEDS are stored in
    tests/golden/ref_fresh_scenes.npz."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mats = [dict(color=tuple(rng.integers(0, 256, 3)), reflection=tuple(rng.integers(0, 200, 3)),
                 transparency=tuple(rng.integers(0, 200, 3)), bump=rng.integers(0, 256, (5, 5, 3)),
                 luminance=tuple(rng.integers(0, 60, 3))) for _ in range(3)]
    lights = [dict(type=int(rng.integers(0, 10)), pos=tuple(rng.uniform(-1, 1, 3)), dir=tuple(rng.uniform(-1, 1, 3)),
                   col=tuple(rng.uniform(0, 1, 3)), radius=float(rng.uniform(0, 1)), half_att=float(rng.choice([np.inf, 1.5])))
              for _ in range(3)]
    return S.make_soup(40, 32, 500, 0.3, seed=seed, samples=2, materials=mats, lights=lights, random_uv=True, smooth_normals=True)


# ---- the opaque-diffuse path class ---------------------------------------------------------------------------------------------
# Scenes the host puts in the opaque-diffuse class (rt_api.cpp materials_admit_opaque_diffuse / lights_admit_opaque_diffuse: every
# reflection, transparency and luminance absent or one black texel, every height map absent or one texel, at most one light), so
# that the GPU renders them with wf_logic_kernel<.., LEAN=true>.  Each aims at one family of that kernel's branches.  The reference's
# planes are stored in tests/golden/ref_class_scenes.npz; tests/test_path_class.py fails if one of them drifts out of the class.

def _img(seed, w, h, lo=0, hi=256):
    """A w x h colour image ([h, w, 3] bytes: mat_size records (w, h))."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(lo, hi, (h, w, 3)).astype(np.uint8)


BLACK = (0, 0, 0)


def class_no_light():
    """No light (:563 loop runs zero times): no shadow ray, the face stays at the ambient 0.1 (:647), and a camera hit's bounce still
    goes out.  White and image colours (bouncing) beside a colour too dark to bounce."""
    mats = [_lambert(), _lambert(color=_img(31, 6, 4)), _lambert(color=(1, 1, 0))]
    return S.make_soup(64, 48, 1500, 0.14, seed=31, samples=2, materials=mats, lights=[], random_uv=True, name="class_no_light")


# One light per scene.  Positional types (1, 2, 7, 8, 9) draw their sphere point before the bounce's (:573 then :671), have a finite
# shadow range and a finite half-attenuation (pow(0.5, d/h) :631); types 1, 7 and 9 sit inside the soup (z 2..4), so N.L changes sign
# across the frame and shadow rays end mid-grid.  Directional types (3-6) draw a point on a spread sphere; type 0 and an unknown type
# draw nothing and leave lmin == lmax == 0 (no shadow ray, :628-636 with N.L = 0).
_CLASS_LIGHTS = {
    0: dict(type=S.LIGHT_OMNI, pos=(0.1, 0.0, 3.0), col=(0.9, 0.8, 0.7)),
    1: dict(type=S.LIGHT_SPOT, pos=(0.1, -0.05, 3.0), col=(0.9, 0.8, 0.7), radius=0.15, half_att=1.5),
    2: dict(type=S.LIGHT_SPOTRECT, pos=(-0.4, 0.3, 1.2), col=(0.6, 0.9, 0.5), radius=0.3, half_att=1.5),
    3: dict(type=S.LIGHT_DISTANT, dir=(-0.6, 0.2, 0.75), col=(0.8, 0.9, 1.0), radius=12.0),
    4: dict(type=S.LIGHT_PARALLEL, dir=(0.1, 0.9, -0.4), col=(1.0, 0.7, 0.5), radius=0.0),
    5: dict(type=S.LIGHT_PARSPOT, dir=(0.7, -0.1, 0.7), col=(0.5, 0.6, 0.9), radius=40.0),
    6: dict(type=S.LIGHT_PARSPOTRECT, dir=(0.0, 0.0, 1.0), col=(0.7, 0.7, 0.7), radius=3.0),
    7: dict(type=S.LIGHT_TUBE, pos=(-0.2, 0.1, 2.6), col=(1.2, 1.0, 0.8), radius=0.05, half_att=1.5),
    8: dict(type=S.LIGHT_AREA, pos=(0.3, -0.2, 1.0), col=(0.9, 1.0, 0.6), radius=0.4, half_att=1.5),
    9: dict(type=S.LIGHT_PHOTOMETRIC, pos=(0.0, 0.2, 3.4), col=(0.8, 0.6, 1.1), radius=0.25, half_att=1.5),
    42: dict(type=42, pos=(0.1, 0.0, 3.0), dir=(0.3, -0.8, 0.5), col=(0.9, 0.8, 0.7), radius=0.3, half_att=1.5),
}


def _class_light(t):
    def make():
        mats = [_lambert(), _lambert(color=_img(40 + t, 5, 5, 40, 256))]
        return S.make_soup(64, 48, 2000, 0.14, seed=40 + t, samples=2, materials=mats, lights=[_CLASS_LIGHTS[t]], random_uv=True,
                           name=f"class_light_type_{t}")
    make.__name__ = f"class_light_type_{t}"
    make.__doc__ = f"One light of type {t} ({_CLASS_LIGHTS[t]})."
    return make


def class_textured_bumped():
    """Image colours of 1x7, 7x1, 5x5 and 8x3 texels and an absent colour (:550, black); one-texel height maps of several values
    (shading_normal's one-texel branch, :231-261); absent and one-black-texel reflection, transparency and luminance side by side;
    smooth normals, wrapping UVs and material -1 on about a fifth of the triangles."""
    mats = [
        dict(color=_img(51, 1, 7), reflection=None, transparency=BLACK, bump=(255, 255, 255), luminance=None),
        dict(color=_img(52, 7, 1), reflection=BLACK, transparency=None, bump=(17, 200, 3), luminance=BLACK),
        dict(color=_img(53, 5, 5), reflection=None, transparency=None, bump=None, luminance=None),
        dict(color=_img(54, 8, 3), reflection=BLACK, transparency=BLACK, bump=(128, 0, 0), luminance=BLACK),
        dict(color=None, reflection=BLACK, transparency=None, bump=(60, 61, 62), luminance=None),
        dict(color=(255, 255, 255), reflection=None, transparency=BLACK, bump=(0, 0, 255), luminance=BLACK),
    ]
    sc = S.make_soup(64, 48, 2500, 0.13, seed=55, samples=2, materials=mats, random_uv=True, smooth_normals=True,
                     lights=[dict(type=S.LIGHT_TUBE, pos=(0.05, 0.05, 2.8), col=(1.1, 0.9, 0.8), radius=0.1, half_att=1.5)],
                     name="class_textured_bumped")
    rng = np.random.Generator(np.random.PCG64(56))
    sc.tri_material[rng.random(sc.triangle_count) < 0.2] = -1
    return sc


def class_degenerate_outside():
    """Triangles collapsed to points and segments (NaN barycentrics meet one-texel colour and height descriptors), the camera
    outside the bounding box, one light bright enough to saturate (:726-741), S=3."""
    mats = [_lambert(), _lambert(color=_img(61, 4, 4), bump=(90, 10, 200))]
    sc = S.make_soup(56, 40, 900, 0.12, seed=61, samples=3, materials=mats, random_uv=True,
                     lights=[dict(type=S.LIGHT_DISTANT, dir=(-0.5, -0.5, 0.2), col=(3.0, 2.0, 40.0))],
                     name="class_degenerate_outside")
    v = sc.vertex.reshape(-1, 3, 4)
    v[::7, 1] = v[::7, 0]
    v[::7, 2] = v[::7, 0]
    v[::11, 2] = v[::11, 1]
    return sc


def class_dark_and_bright():
    """Colours on both sides of the bounce threshold 3/256 <= w.x + w.y + w.z (:664): (1,1,1) bounces, (1,1,0) and (2,0,0) do not,
    so paths of both shapes share waves; one positional light with a negative colour channel."""
    mats = [_lambert(color=(1, 1, 1)), _lambert(color=(1, 1, 0)), _lambert(color=(2, 0, 0)), _lambert(),
            _lambert(color=_img(71, 3, 3, 0, 3))]
    return S.make_soup(64, 48, 2000, 0.13, seed=71, samples=2, materials=mats, random_uv=True,
                       lights=[dict(type=S.LIGHT_AREA, pos=(0.2, 0.1, 2.9), col=(-0.4, 0.7, 1.5), radius=0.2, half_att=2.5)],
                       name="class_dark_and_bright")


CLASS = [class_no_light] + [_class_light(t) for t in list(range(10)) + [42]] + [class_textured_bumped, class_degenerate_outside,
                                                                                  class_dark_and_bright]


def class_by_name(name):
    for f in CLASS:
        if f.__name__ == name:
            return f
    raise KeyError(name)


# ---- fuzz scenes (tests/test_fuzz_parity_gpu.py, tests/fuzz_parity.py) --------------------------------------------------------

def fuzz_scene(seed):
    """A random soup drawn from the seed alone.  Even seeds draw an opaque-diffuse class scene: zero or one light of any type,
    reflection, transparency and luminance absent or black, a height map absent or one texel of any value, material -1 on some
    triangles.  Odd seeds draw a general scene: textures, bump maps, mirrors, transparency, glow and up to four lights."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nm = int(rng.integers(1, 6))

    def image():
        return rng.integers(0, 256, (int(rng.integers(1, 9)), int(rng.integers(1, 9)), 3))

    if seed % 2 == 0:
        def absent_or_black():
            return None if rng.integers(0, 2) else BLACK
        mats = []
        for _ in range(nm):
            colour = (None, tuple(rng.integers(0, 256, 3)), image())[int(rng.integers(0, 3))]
            bump = None if rng.integers(0, 2) else tuple(rng.integers(0, 256, 3))
            mats.append(dict(color=colour, reflection=absent_or_black(), transparency=absent_or_black(), bump=bump,
                             luminance=absent_or_black()))
        nl = int(rng.integers(0, 4) > 0)  # (one light three times in four)
    else:
        mats = [dict(color=image(), reflection=tuple(rng.integers(0, 200, 3)), transparency=tuple(rng.integers(0, 200, 3)), bump=image(),
                     luminance=tuple(rng.integers(0, 60, 3))) for _ in range(nm)]
        nl = int(rng.integers(0, 5))
    lights = [dict(type=int(t), pos=tuple(rng.uniform(-1, 1, 3) + [0, 0, 2]), dir=tuple(rng.uniform(-1, 1, 3)), col=tuple(rng.uniform(0, 1, 3)),
                   radius=float(rng.uniform(0, 1)), half_att=float(rng.choice([np.inf, 2.5, 0.7]))) for t in rng.integers(0, 11, nl)]
    w, h = int(rng.integers(60, 321)), int(rng.integers(40, 241))
    tris, edge = int(rng.integers(200, 20001)), float(rng.choice([0.01, 0.03, 0.08, 0.2]))
    sc = S.make_soup(w, h, tris, edge, seed=seed, samples=int(rng.integers(1, 5)), materials=mats, lights=lights, random_uv=True,
                     smooth_normals=bool(rng.integers(0, 2)), name=f"fuzz_{seed}")
    if seed % 2 == 0 and rng.integers(0, 2):
        sc.tri_material[rng.random(sc.triangle_count) < 0.15] = -1
    sc.meta.update(materials=nm, lights=[int(t) for t in sc.light_type], path_class="opaque-diffuse" if seed % 2 == 0 else "general")
    return sc


def fuzz_summary(sc):
    m = sc.meta
    return (f"seed {m['seed']}: {sc.width}x{sc.height}, {sc.triangle_count} triangles (edge {m['edge']}), {m['materials']} materials, "
            f"light types {m['lights']}, S={sc.sample_count}, drawn as {m['path_class']}")


def by_name(name):
    for f in ALL:
        if f.__name__ == name:
            return f
    raise KeyError(name)


# ---- AXIS: grid walks with zero and extreme direction components --------------------------------------------------------------
# Mesh rooms of axis-aligned quads at exactly representable coordinates (many vertices share a coordinate: repeated split planes,
# zero-width cells, hits exactly on a plane), lit by lights along or next to an axis with radius 0.  A directional light's shadow
# direction is GetSpherePoint(r = 0) - dir (:589-606): every zero component of dir comes out +0 or -0 by the sign of that hit's
# random draw, so the walk meets 0 <= -0.0, heads of -inf and NaN (0/0 on a plane) and steps along a zero axis (:383-395).
# The reference's planes are stored in tests/golden/ref_axis_scenes.npz; tests/test_walk_edges.py checks with the oracle's walk
# census (rt_oracle_render_census) that every scene still meets the edge it is named for.

from opencl_render_amd import demo as _demo, frontend as _F  # noqa: E402  (the AXIS scenes are mesh scenes)

TAME_LO, TAME_HI = 2.0 ** -60, 2.0 ** 39  # rt_api.cpp: a plane coordinate is tame when it is 0 or in [2^-60, 2^39]


def planes_tame(box_min):
    m = np.abs(np.asarray(box_min, np.float32)[:, :3])
    return bool(np.all((m == 0) | ((m >= np.float32(TAME_LO)) & (m <= np.float32(TAME_HI)))))


def repeated_planes(box_min):
    """Split planes equal to the one before them, over the three axes (each is a cell of zero width)."""
    b = np.asarray(box_min, np.float32)[:, :3]
    return int((b[1:] == b[:-1]).sum())


def _panel(axis, value, lo, hi, step, material):
    """An axis-aligned rectangle at coordinate `value` of `axis`, spanning lo..hi (the other two axes in order) in square quads of
    side `step`: every vertex at an exact multiple of step."""
    u = np.arange(lo[0], hi[0] + step / 2, step, dtype=np.float64)
    v = np.arange(lo[1], hi[1] + step / 2, step, dtype=np.float64)
    others = [a for a in range(3) if a != axis]
    pts = np.zeros((len(v), len(u), 3))
    pts[..., axis] = value
    pts[..., others[0]] = u[None, :]
    pts[..., others[1]] = v[:, None]
    nu = len(u)
    quads = [[j * nu + i, j * nu + i + 1, (j + 1) * nu + i + 1, (j + 1) * nu + i] for j in range(len(v) - 1) for i in range(nu - 1)]
    quads = np.array(quads, np.int32)
    uv = np.tile(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), (len(quads), 1, 1))
    return _F.Mesh(points=pts.reshape(-1, 3).astype(np.float32), polygons=quads, corner_uv=uv,
                   polygon_material=np.full(len(quads), material, np.int32))


ROOM_LO, ROOM_HI = (-2.0, 0.0, 0.5), (2.0, 2.5, 5.0)


def _room_meshes(floor=0, walls=0, ceiling=False, props=1, step=0.25):
    """Floor, back wall, left and right walls (and a ceiling) of the box ROOM_LO..ROOM_HI, open towards the camera, plus two boxes and
    a pyramid standing on the floor (material `props`)."""
    (x0, y0, z0), (x1, y1, z1) = ROOM_LO, ROOM_HI
    m = [_panel(1, y0, (x0, z0), (x1, z1), step, floor), _panel(2, z1, (x0, y0), (x1, y1), 2 * step, walls),
         _panel(0, x0, (y0, z0), (y1, z1), 2 * step, walls), _panel(0, x1, (y0, z0), (y1, z1), 2 * step, walls)]
    if ceiling:
        m.append(_panel(1, y1, (x0, z0), (x1, z1), 4 * step, walls))
    m += [_demo.quad_box((-1.25, 0.0, 2.0), (-0.5, 0.75, 2.75), props), _demo.quad_box((0.5, 0.0, 3.0), (1.25, 1.5, 3.5), props),
          _demo.pyramid([(0.0, 0.0, 1.5), (0.5, 0.0, 1.5), (0.5, 0.0, 2.0), (0.0, 0.0, 2.0)], (0.25, 0.5, 1.75), props)]
    return m


def _axis_scene(name, lights, width=96, height=72, samples=2, materials=None, meshes=None, scale=1.0, extra=None):
    """A room scene through the front-end, then the lights packed as given (radius and direction bits untouched: rtHipLightFill would
    normalise the direction and set the radius to 0.52) and the host builders' lists."""
    meshes = _room_meshes() if meshes is None else meshes
    if scale != 1.0:
        meshes = [_F.Mesh(points=(np.asarray(mm.points, np.float64) * scale).astype(np.float32), polygons=mm.polygons,
                          corner_uv=mm.corner_uv, polygon_material=mm.polygon_material) for mm in meshes]
    meshes = meshes + (extra or [])
    mats = materials or [dict(rgb=(0.8, 0.8, 0.75)), dict(rgb=(0.9, 0.5, 0.3))]
    sc = _F.scene_from_meshes(meshes, mats, [], position=(0.25 * scale, 1.25 * scale, -2.0 * scale), look_at=(0.0, 0.75 * scale, 3.0 * scale),
                              up=(0, 1, 0), fov=np.radians(60.0), width=width, height=height, samples=samples, name=name)
    sc.light_type, sc.light_pos, sc.light_dir, sc.light_col, sc.light_radius, sc.light_half_att = S.pack_lights(lights)
    R.build_lists(sc)
    return sc


def _check(sc, tame=True, min_repeated=100):
    assert planes_tame(sc.box_min) == tame, f"{sc.name}: planes tame = {planes_tame(sc.box_min)}"
    assert repeated_planes(sc.box_min) >= min_repeated, f"{sc.name}: {repeated_planes(sc.box_min)} repeated planes"
    return sc


def _sun(t, d, col=0.3, radius=0.0):
    return dict(type=t, dir=d, col=(col, col, col), radius=radius)


AXES = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]


def _axis_suns(t):
    def make():
        sc = _check(_axis_scene(f"axis_suns_type_{t}", [_sun(t, d, 0.18) for d in AXES]))
        zeros = sc.light_dir[:, :3] == 0
        assert zeros.sum() == 12 and not np.signbit(sc.light_dir[:, :3][zeros]).any() and (sc.light_radius == 0).all()
        return sc
    make.__name__ = f"axis_suns_type_{t}"
    make.__doc__ = f"Six radius-0 lights of type {t}, along +x, -x, +y, -y, +z and -z: every shadow direction has two +-0 components."
    return make


def axis_sun_negative_zero_dir():
    """A sun straight overhead written (-0.0, -1, -0.0): (+-0) - (-0) = +0, so every zero of its shadow direction is +0 (a branch the
    +0 spelling does not take), beside a sun along +x written (1, +0, +0) and one written (1, -0.0, -0.0)."""
    sc = _check(_axis_scene("axis_sun_negative_zero_dir", [_sun(3, (-0.0, -1.0, -0.0), 0.4), _sun(4, (1.0, 0.0, 0.0), 0.3),
                                                            _sun(4, (1.0, -0.0, -0.0), 0.3)]))
    assert np.signbit(sc.light_dir[0, [0, 2]]).all() and not np.signbit(sc.light_dir[1, 1:3]).any() and np.signbit(sc.light_dir[2, 1:3]).all()
    return sc


def axis_planes_fine():
    """Floor and walls in quads of 1/8: hundreds of repeated planes, hits that land exactly on them (0/0 heads), a ceiling, lit by a
    sun along -y (blocked by the ceiling: the walks end at a hit) and a sun along -z through the open front."""
    sc = _axis_scene("axis_planes_fine", [_sun(4, (0.0, -1.0, 0.0), 0.4), _sun(3, (0.0, 0.0, 1.0), 0.4)],
                     meshes=_room_meshes(ceiling=True, step=0.125))
    return _check(sc, min_repeated=400)


NEAR_AXIS = (2.0 ** -40, 1e-13, 1e-40, 2.0 ** -149)


def axis_near_axis_lights():
    """Suns whose directions have one component of 2^-40 (the fast quotient's bound), 1e-13, 1e-40 (subnormal) and 2^-149 (the smallest
    subnormal) next to an axis: finite, non-zero, but not tame, so no wave takes the short quotient."""
    lights = [_sun(3, (e, -1.0, 0.0), 0.2) for e in NEAR_AXIS] + [_sun(4, (0.0, -e, 1.0), 0.2) for e in NEAR_AXIS[::-1]]
    sc = _check(_axis_scene("axis_near_axis_lights", lights))
    assert sc.light_dir[3, 0] == np.float32(2.0 ** -149) and sc.light_dir[2, 0] < np.finfo(np.float32).tiny
    return sc


def axis_near_axis_mixed():
    """The near-axis suns beside ordinary lights in the same frame (tame and non-tame shadow rays share waves), 200x150: more than one
    128x128 tile."""
    lights = [_sun(3, (0.3, -0.8, 0.5), 0.3, radius=2.0), _sun(4, (2.0 ** -40, -1.0, -1e-40), 0.3), _sun(5, (1e-13, 2.0 ** -149, 1.0), 0.3),
              dict(type=S.LIGHT_SPOT, pos=(0.3, 2.0, 1.5), col=(0.4, 0.4, 0.4), radius=0.1)]
    return _check(_axis_scene("axis_near_axis_mixed", lights, width=200, height=150))


def _far_triangle(c):
    return _F.Mesh(points=np.array([[c, 0, c], [c + 1, 0, c], [c, 1, c]], np.float32), polygons=np.array([[0, 1, 2, 2]], np.int32))


def _specks(size, at=(0.0, 0.0, 0.0), n=64):
    """n tiny triangles of side `size` at `at`: their vertex coordinates become split planes."""
    pts, pol = [], []
    for k in range(n):
        o = np.asarray(at, np.float64) + size * k
        pts += [o, o + (size, 0, 0), o + (0, size, size)]
        pol.append([3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 2])
    return [_F.Mesh(points=np.array(pts, np.float32), polygons=np.array(pol, np.int32))]


def axis_untame_far():
    """The room with one far triangle at 1e12 (beyond 2^39): planesTame == 0, every wave divides the long way."""
    sc = _axis_scene("axis_untame_far", [_sun(4, (0.0, -1.0, 0.0), 0.4), _sun(3, (1.0, 0.0, 0.0), 0.3)], extra=[_far_triangle(1e12)])
    return _check(sc, tame=False)


def axis_untame_tiny():
    """The room with 64 specks of 2^-70 at the origin (plane coordinates non-zero below 2^-60): planesTame == 0."""
    sc = _axis_scene("axis_untame_tiny", [_sun(4, (0.0, -1.0, 0.0), 0.4), _sun(6, (0.0, 0.0, 1.0), 0.3)], extra=_specks(2.0 ** -70))
    return _check(sc, tame=False)


def axis_untame_scaled():
    """The room scaled by 2^30 (its triangle test still far from overflow) with a speck of side 2^-40 at its origin: planes span
    2^-40 .. 2^32.3 and are not tame."""
    sc = _axis_scene("axis_untame_scaled", [_sun(4, (0.0, -1.0, 0.0), 0.4), _sun(5, (-1.0, 0.0, 0.0), 0.3)], scale=2.0 ** 30,
                     extra=_specks(2.0 ** -64))
    return _check(sc, tame=False)


def axis_tame_bounds():
    """Plane coordinates exactly at the tame bounds: 64 point triangles at (2^-60, 2^-60, 2^-60) and a far triangle at 2^39 (its other
    corners 2^39 + 1 round back to 2^39): still tame."""
    sc = _axis_scene("axis_tame_bounds", [_sun(4, (0.0, -1.0, 0.0), 0.4), _sun(3, (0.0, 0.0, -1.0), 0.3)],
                     extra=_specks(0.0, at=(2.0 ** -60, 2.0 ** -60, 2.0 ** -60)) + [_far_triangle(2.0 ** 39)])
    m = np.abs(sc.box_min[:, :3])
    assert m.max() == np.float32(2.0 ** 39) and m[m > 0].min() == np.float32(2.0 ** -60)
    return _check(sc, tame=True)


def axis_point_lights():
    """Point-type lights (1, 2, 7, 8, 9) of radius 0: on the left wall's plane, at the grid's corner, outside the box along an axis
    (above, behind the back wall, beside the right wall).  Finite shadow rays whose end point lies on a plane or outside the box meet
    BindInCube's '<= 0' tests with zero components."""
    (x0, y0, z0), (x1, y1, z1) = ROOM_LO, ROOM_HI
    lights = [dict(type=1, pos=(x0, 1.25, 2.5), col=(0.3, 0.3, 0.3), radius=0.0, half_att=3.0),
              dict(type=2, pos=(x0, y0, z0), col=(0.3, 0.3, 0.3), radius=0.0),
              dict(type=7, pos=(0.25, 6.0, 2.5), col=(0.3, 0.3, 0.3), radius=0.0),
              dict(type=8, pos=(0.25, 1.25, 9.0), col=(0.3, 0.3, 0.3), radius=0.0, half_att=5.0),
              dict(type=9, pos=(7.0, 0.75, 3.0), col=(0.3, 0.3, 0.3), radius=0.0)]
    return _check(_axis_scene("axis_point_lights", lights))


def axis_mirror_glass():
    """A mirror floor and a glass box in the axis room: bounce and see-through rays cross the same planes, S=3."""
    mats = [dict(rgb=(0.7, 0.7, 0.7), reflection=np.full((1, 1, 3), 200, np.uint8)), dict(rgb=(0.8, 0.8, 0.75)),
            dict(rgb=(0.8, 0.9, 1.0), transparency=np.full((1, 1, 3), 170, np.uint8))]
    sc = _axis_scene("axis_mirror_glass", [_sun(4, (0.0, -1.0, 0.0), 0.4), _sun(3, (-1.0, 0.0, 0.0), 0.3)], samples=3, materials=mats,
                     meshes=_room_meshes(floor=0, walls=1, props=2))
    return _check(sc)


def axis_class_sun():
    """One radius-0 sun along -y over a white room: the opaque-diffuse class (wf_logic_kernel<.., LEAN=true>), 160x120."""
    sc = _axis_scene("axis_class_sun", [_sun(4, (0.0, -1.0, 0.0), 0.8)], width=160, height=120,
                     materials=[dict(rgb=(0.8, 0.8, 0.75)), dict(rgb=(0.6, 0.7, 0.9))])
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE
    return _check(sc)


AXIS = [_axis_suns(t) for t in (3, 4, 5, 6)] + [axis_sun_negative_zero_dir, axis_planes_fine, axis_near_axis_lights, axis_near_axis_mixed,
                                                 axis_untame_far, axis_untame_tiny, axis_untame_scaled, axis_tame_bounds, axis_point_lights,
                                                 axis_mirror_glass, axis_class_sun]


def axis_by_name(name):
    for f in AXIS:
        if f.__name__ == name:
            return f
    raise KeyError(name)


def axis_fuzz_scene(seed):
    """A random axis room drawn from the seed alone: boxes on a quarter grid, floor quads of 1/4 or 1/8, with or without a ceiling,
    1-3 lights along an axis or next to one (zero components written +0 or -0, near-axis components from NEAR_AXIS), radius 0 or not,
    one point light in one seed of two, S 1-3, up to 160x120."""
    rng = np.random.Generator(np.random.PCG64(seed))
    meshes = _room_meshes(ceiling=bool(rng.integers(0, 2)), step=float(rng.choice([0.25, 0.125])))[:-3]  # random boxes for the props
    for _ in range(int(rng.integers(1, 6))):
        lo = np.array([rng.integers(-7, 6) / 4, 0.0, rng.integers(4, 18) / 4])
        hi = lo + np.array([rng.integers(1, 5) / 4, rng.integers(1, 9) / 4, rng.integers(1, 5) / 4])
        meshes.append(_demo.quad_box(tuple(lo), tuple(hi), int(rng.integers(0, 3))))
    lights = []
    for _ in range(int(rng.integers(1, 4))):
        d = np.array(AXES[int(rng.integers(0, 6))])
        a = int(np.nonzero(d)[0][0])
        for k in range(3):
            if k != a:
                d[k] = (-0.0 if rng.integers(0, 2) else 0.0) if rng.integers(0, 3) else float(rng.choice(NEAR_AXIS)) * rng.choice([-1, 1])
        lights.append(_sun(int(rng.integers(3, 7)), tuple(d), 0.3, radius=float(rng.choice([0.0, 0.0, 1.5]))))
    if seed % 2:
        lights.append(dict(type=int(rng.choice([1, 2, 7, 8, 9])), pos=(rng.integers(-8, 9) / 4, rng.integers(0, 11) / 4, rng.integers(2, 21) / 4),
                           col=(0.3, 0.3, 0.3), radius=0.0))
    mats = [dict(rgb=(0.8, 0.8, 0.75)), dict(rgb=(0.9, 0.5, 0.3)),
            dict(rgb=(0.8, 0.9, 1.0), transparency=np.full((1, 1, 3), int(rng.integers(0, 200)), np.uint8),
                 reflection=np.full((1, 1, 3), int(rng.integers(0, 120)), np.uint8))]
    w, h = int(rng.integers(48, 161)), int(rng.integers(36, 121))
    sc = _axis_scene(f"axis_fuzz_{seed}", lights, width=w, height=h, samples=int(rng.integers(1, 4)), materials=mats, meshes=meshes)
    sc.meta.update(seed=seed, lights=[(int(t), tuple(float(v) for v in d[:3])) for t, d in zip(sc.light_type, sc.light_dir)])
    return sc


def axis_fuzz_summary(sc):
    return f"seed {sc.meta['seed']}: {sc.width}x{sc.height}, {sc.triangle_count} triangles, S={sc.sample_count}, lights {sc.meta['lights']}"


# ---- shading known answers (tests/golden/kat_shading.npz, tests/test_shading_kat.py, tests/test_shading_kat_gpu.py) ------------------
# The texel look-up (raytrace_opencl.c:103-122) and the shading normal (:195-263) on resident scenes.  The tables are generated from a
# formula (bytes of an integer hash of the texel index), so that the fixture stores only the queries and the reference's answers.

def hash_texels(n, salt):
    """n texels [n, 4] u8 (the 4th byte 0): the low three bytes of splitmix64(index + salt * golden ratio)."""
    x = np.arange(n, dtype=np.uint64) + np.uint64((salt * 0x9E3779B97F4A7C15) & (2 ** 64 - 1))
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    out = np.zeros((n, 4), np.uint8)
    out[:, :3] = x.view(np.uint8).reshape(n, 8)[:, :3]
    return out


# (w, h) of the texel scene's tables, in atlas order: the small shapes, then a 4096 x 4096 table, so that the last table starts above
# 2^24 texels.  Table i is channel i % 5 of material i (the other channels absent).
TEXEL_TABLES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (64, 48), (1024, 1), (1, 1024), (4096, 4096), (37, 29)]


def shade_texel_scene():
    """A few triangles whose materials carry TEXEL_TABLES (the triangles themselves are not queried)."""
    m = len(TEXEL_TABLES)
    sc = S.make_soup(32, 24, 40, 0.2, seed=81, samples=1, materials=[_lambert()] * m, name="shade_texel_scene")
    sizes = np.zeros((S.CH_COUNT * m, 2), np.uint32)
    starts = np.zeros(S.CH_COUNT * m + 1, np.int32)
    cursor = 0
    for i, (w, h) in enumerate(TEXEL_TABLES):
        for c in range(S.CH_COUNT):
            starts[S.CH_COUNT * i + c] = cursor
            if c == i % S.CH_COUNT:
                sizes[S.CH_COUNT * i + c] = (w, h)
                cursor += w * h
    starts[-1] = cursor
    sc.mat_size, sc.mat_start = sizes, starts
    sc.textures = np.concatenate([hash_texels(w * h, 1000 + i) for i, (w, h) in enumerate(TEXEL_TABLES)])
    return sc


# Materials of the normal scenes: none (-1 is assigned on top), no height map, one-texel height maps of several values, and image
# height maps of 1x7, 7x1, 5x5 and 64x48 texels.  NORMAL_BUMPS[i] is material i's height map.
NORMAL_BUMPS = [None, (255, 0, 0), (17, 3, 9), (128, 128, 128), (0, 0, 0), (1, 7), (7, 1), (5, 5), (64, 48)]


def _bump_image(w, h, salt):
    return hash_texels(w * h, salt)[:, :3].reshape(h, w, 3)


def shade_normal_scene(zoom=1):
    """A soup with smooth, flat and non-unit vertex normals and some collapsed triangles, UVs spread wide so that neighbouring pixels
    land on different texels of the height maps; every tenth triangle lies in the plane z = 3 (the camera's tb and lr have no z, so
    probe rays with d.z = 0 are parallel to it).  zoom = 1: a 60-pixel-wide camera (pixelSizeInv 60); zoom = 50: the same view
    magnified 50 times (pixelSizeInv 3000, tb and lr 50 times shorter)."""
    mats = []
    for i, b in enumerate(NORMAL_BUMPS):
        bump = None if b is None else (_bump_image(b[0], b[1], 2000 + i) if i >= 5 else b)
        mats.append(dict(color=(200, 200, 200), bump=bump))
    t = 360
    sc = S.make_soup(60, 44, t, 0.35, seed=91, samples=1, materials=mats, random_uv=True, smooth_normals=True,
                     material_ids=(np.arange(t) % (len(mats) + 1) - 1).astype(np.int32), name=f"shade_normal_scene_{zoom}")
    rng = np.random.Generator(np.random.PCG64(92))
    sc.tri_uv *= np.float32(9.0)
    nrm = sc.tri_normal.reshape(t, 3, 4)
    v = sc.vertex.reshape(t, 3, 4)
    flat = np.arange(t) % 3 == 1
    nrm[flat, 1:] = nrm[flat, :1]
    scaled = np.arange(t) % 3 == 2
    nrm[scaled, :, :3] *= rng.uniform(0.2, 5.0, (int(scaled.sum()), 3, 1)).astype(np.float32)
    planar = np.arange(t) % 10 == 4
    v[planar, :, 2] = np.float32(3.0)
    a = v[planar, 0, :3]
    n = np.cross(v[planar, 1, :3] - a, v[planar, 2, :3] - a)
    nrm[planar, :, :3] = np.where(n[:, 2:3] < 0, np.float32(-1), np.float32(1))[:, None, :] * np.array([0, 0, 1], np.float32)
    v[np.arange(t) % 23 == 7, 2] = v[np.arange(t) % 23 == 7, 1]           # segments
    v[np.arange(t) % 29 == 11, 1:] = v[np.arange(t) % 29 == 11, :1]      # points
    if zoom != 1:
        z = np.float32(zoom)
        sc.left_to_right = (sc.left_to_right / z).astype(np.float32)
        sc.top_to_bottom = (sc.top_to_bottom / z).astype(np.float32)
        sc.eye_to_top_left = (sc.eye_to_top_left * np.array([1 / z, 1 / z, 1, 0], np.float32)).astype(np.float32)
        sc.pixel_size_inv = float(np.float32(sc.pixel_size_inv) * z)
    return sc


# light spreads the host computes for sun radii 0, 0.5, 90 and 360 degrees (rt_api.cpp, raytrace_opencl.c:594) are minted with these
# light directions
SPREAD_RADII = (0.0, 0.5, 90.0, 360.0)
SPREAD_DIRS = ((0.3, -0.8, 0.5), (0.0, 0.0, 2.0))


# ---- slots out of image order over partial tiles: what every read-back of a tile buffer has to place right ----------------------------
SHUFFLED_TILES = (3, 0)  # of the 2 x 2 tiles of shuffled_tiles(): the ragged corner tile (32 x 16 pixels of it in the image) first, then a whole one


def shuffled_tiles():
    """160 x 144: two tiles across and two down, ragged on both edges; 300 triangles, two samples per pixel.  Rendered as the tiles
    SHUFFLED_TILES, slot order and image order differ and one slot is mostly outside the image."""
    return R.build_lists(S.make_soup(160, 144, 300, 0.3, seed=41, samples=2, name="shuffled_tiles"))


def tiles_mask(sc, tiles):
    """[H, W] bool: the pixels of `tiles`."""
    mine = np.zeros((sc.height, sc.width), bool)
    for t in tiles:
        ty, tx = divmod(int(t), (sc.width + R.TILE - 1) // R.TILE)
        mine[ty * R.TILE:(ty + 1) * R.TILE, tx * R.TILE:(tx + 1) * R.TILE] = True
    return mine
