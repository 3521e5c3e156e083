"""What the scene-edit tests (tests/test_scene_edit_gpu.py) and the session model (tests/session_cases.py) both need: light and material
sets as the arrays an edit takes, the twin of a Scene with such fields replaced, and material ids folded into a table's range."""
import copy

import numpy as np

from opencl_render_amd import raytrace as R, scene as S


def lights_of(spec):
    """The six arrays (a dict under Scene's field names) of a list of light dicts, or of a Scene."""
    return R.scene_lights(spec) if isinstance(spec, S.Scene) else dict(zip(R.LIGHT_FIELDS, S.pack_lights(spec)))


def materials_of(spec):
    if isinstance(spec, S.Scene):
        return dict(mat_size=spec.mat_size, mat_start=spec.mat_start, textures=spec.textures)
    return dict(zip(("mat_size", "mat_start", "textures"), S.pack_materials(spec)))


def twin_of(sc, lights=None, materials=None, ids=None, **fields):
    out = copy.copy(sc)
    for part in (lights, materials):
        for k, v in (part or {}).items():
            setattr(out, k, v)
    if ids is not None:
        out.tri_material = np.ascontiguousarray(ids, np.int32)
    for k, v in fields.items():
        setattr(out, k, v)
    return out


def many_lights(n, seed):
    """n dim lights of types 0..9 inside and around the soup (dim: their sum stays below saturation)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [dict(type=int(rng.integers(0, 10)), pos=tuple(rng.uniform(-1, 1, 3) + [0, 0, 2]), dir=tuple(rng.uniform(-1, 1, 3)),
                 col=tuple(rng.uniform(0.004, 0.03, 3)), radius=float(rng.uniform(0.05, 0.6)), half_att=float(rng.choice([np.inf, 2.0])))
            for _ in range(n)]


def fold(ids, m):
    ids = np.asarray(ids, np.int32)
    return np.where(ids < 0, ids, ids % m).astype(np.int32)


ONE_SUN = [dict(type=S.LIGHT_DISTANT, dir=(0.3, -0.8, 0.5), col=(0.9, 0.9, 0.8))]
SPOT = dict(type=S.LIGHT_SPOT, pos=(0.4, 0.6, 1.5), col=(0.5, 0.4, 0.3), radius=0.2, half_att=2.0)
