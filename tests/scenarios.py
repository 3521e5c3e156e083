"""Seeded parity scenarios shared by the golden-fixture generator, the oracle tests and the GPU parity tests.

Each scenario is small enough for the single-thread oracle to finish in well under a second and is aimed at one
part of the reference kernel (raytrace_opencl.c line ranges in the comments).  Inputs are deterministic functions
of the seed (numpy PCG64); the golden fixtures nevertheless store the inputs themselves (tests/golden/*.npz).
"""
from __future__ import annotations

import numpy as np

from opencl_render_amd import scene as S


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
