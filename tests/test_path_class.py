"""Which logic kernel a scene's paths run on (rtHipScenePathClass, rt_api.cpp path_class_of), decided on the host: the
opaque-diffuse class (no reflection, transparency or luminance other than absent or one black texel, no image height map, at
most one light) or the general one.  No GPU needed."""
import copy

import numpy as np
import pytest

import scenarios as SC
from opencl_render_amd import raytrace as R, scene as S

LAMBERT = dict(color=(255, 255, 255), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0))


def _with_materials(sc, materials):
    sc = copy.copy(sc)
    sc.mat_size, sc.mat_start, sc.textures = S.pack_materials(materials)
    sc.tri_material = np.zeros(sc.triangle_count, np.int32)
    return sc


def _with_lights(sc, lights):
    sc = copy.copy(sc)
    sc.light_type, sc.light_pos, sc.light_dir, sc.light_col, sc.light_radius, sc.light_half_att = S.pack_lights(lights)
    return sc


def _soup():
    return S.make_soup(64, 48, 500, 0.06, seed=3)


def test_opaque_diffuse_scenes():
    assert R.path_class(_soup()) == R.PATH_CLASS_OPAQUE_DIFFUSE  # make_soup's default: white Lambert, one-texel black bump, one distant light
    assert R.path_class(SC.lambert_distant()) == R.PATH_CLASS_OPAQUE_DIFFUSE
    no_mat = _soup()
    no_mat.tri_material = np.full(no_mat.triangle_count, -1, np.int32)  # material -1 everywhere (scenarios.no_material's own table has images)
    assert R.path_class(no_mat) == R.PATH_CLASS_OPAQUE_DIFFUSE
    assert R.path_class(_with_lights(_soup(), [])) == R.PATH_CLASS_OPAQUE_DIFFUSE
    rng = np.random.Generator(np.random.PCG64(1))
    image = rng.integers(0, 256, (4, 4, 3)).astype(np.uint8)
    assert R.path_class(_with_materials(_soup(), [dict(LAMBERT, color=image), dict(LAMBERT, bump=(9, 200, 31))])) == R.PATH_CLASS_OPAQUE_DIFFUSE
    for t in list(range(10)) + [42]:  # one light of any type
        assert R.path_class(_with_lights(_soup(), [dict(type=t, pos=(0, 0, 1), dir=(0.2, -0.5, 0.8), col=(1, 1, 1), radius=0.2)])) == R.PATH_CLASS_OPAQUE_DIFFUSE


def test_general_scenes():
    for make in (SC.mirror_hall, SC.mixed_materials_textured, SC.all_light_types, SC.primary_only, SC.no_material):
        assert R.path_class(make()) == R.PATH_CLASS_GENERAL, make.__name__
    rng = np.random.Generator(np.random.PCG64(2))
    image = rng.integers(0, 256, (4, 4, 3)).astype(np.uint8)
    assert R.path_class(_with_materials(_soup(), [LAMBERT, dict(LAMBERT, bump=image)])) == R.PATH_CLASS_GENERAL
    two = [dict(type=S.LIGHT_DISTANT, dir=(0.2, -0.5, 0.8), col=(1, 1, 1)), dict(type=S.LIGHT_DISTANT, dir=(-0.2, -0.5, 0.8), col=(1, 1, 1))]
    assert R.path_class(_with_lights(_soup(), two)) == R.PATH_CLASS_GENERAL
    for ch in ("reflection", "transparency", "luminance"):  # one texel that is not black
        assert R.path_class(_with_materials(_soup(), [dict(LAMBERT, **{ch: (0, 0, 1)})])) == R.PATH_CLASS_GENERAL, ch


@pytest.mark.parametrize("name", [f.__name__ for f in SC.CLASS])
def test_class_scenarios_stay_in_the_class(name):
    """Every scenario the class tests pin (scenarios.CLASS) must run the opaque-diffuse kernel: one that drifted out of the class would
    quietly test the general kernel instead."""
    assert R.path_class(SC.class_by_name(name)()) == R.PATH_CLASS_OPAQUE_DIFFUSE


def test_even_fuzz_seeds_draw_class_scenes():
    for seed in range(0, 64, 2):
        assert R.path_class(SC.fuzz_scene(seed)) == R.PATH_CLASS_OPAQUE_DIFFUSE, SC.fuzz_summary(SC.fuzz_scene(seed))
