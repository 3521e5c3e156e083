"""The grid walk where ray directions have zero or extreme components, on the CPU: the oracle against the reference kernel.

scenarios.AXIS holds mesh rooms of axis-aligned quads lit by lights along or next to an axis with radius 0 (see scenarios.py).  Their
inputs are where a DDA goes wrong: direction components of +0 and -0 (the walk's 0 <= d picks the upper plane for -0.0 too, and
(plane - o) / -0.0 is -inf), heads of 0/0 where an origin lies on a split plane, zero-width cells, steps along a zero axis until the
walk leaves the grid, components below the fast quotient's bound (2^-40) down to the smallest subnormal, planes outside the tame
range, and finite shadow rays whose end point BindInCube clamps with zero components.

Here the oracle's walk census (rt_oracle_render_census) shows that every scene still meets the edge it is named for, and the
oracle's planes must equal the reference kernel's (tests/golden/ref_axis_scenes.npz, and the kernel itself where oracle/_ref was
built) bit for bit.  The GPU side is tests/test_walk_edges_gpu.py.  Nothing here renders with the product library."""
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import scenarios as SC
from conftest import GOLDEN

AXIS_NAMES = [f.__name__ for f in SC.AXIS]
THREADS = min(os.cpu_count() or 1, 16)

# Lower bounds on the census counters each scene is there for.  Measured values when the floors were set are in the comments; the
# floors are about half of them, so that a change of camera or tessellation that keeps the edge does not trip them, and a change that
# loses it does.
_SUNS = dict(dir_pos_zero=50_000, dir_neg_zero=50_000, origin_on_plane=50_000, head_nan=30_000, head_neg_inf=35_000, head_pos_inf=35_000,
             zero_axis_steps=3_500_000, end_left_grid=40_000, end_hit=14_000, zero_width_start=30_000, bind_zero_outside=800)
# axis_suns_type_*: 107708 +0, 106768 -0, 106974 on a plane, 64436 NaN, 74616 -inf, 75424 +inf heads, 7383241 zero-axis steps,
# 89026 left the grid, 29714 hits, 60238 zero-width starts, 1732 zero components outside the box
FLOORS = {f"axis_suns_type_{t}": _SUNS for t in (3, 4, 5, 6)}
FLOORS.update({
    # 90056 +0, 17902 -0 (the +x sun written +0), 29301 NaN, 13663 -inf, 2934916 zero-axis steps
    "axis_sun_negative_zero_dir": dict(dir_pos_zero=45_000, dir_neg_zero=8_000, head_nan=14_000, head_neg_inf=6_500, zero_axis_steps=1_400_000),
    # 56492 origins on a plane, 29774 NaN heads, 25095 zero-width starts, 18588 hits (the ceiling)
    "axis_planes_fine": dict(origin_on_plane=28_000, head_nan=14_000, zero_width_start=12_000, end_hit=9_000, dir_neg_zero=24_000),
    # 107322 untame and 71548 subnormal components, 71181 -0
    "axis_near_axis_lights": dict(dir_untame=50_000, dir_subnormal=35_000, dir_neg_zero=35_000, head_pos_inf=50_000),
    # 232272 untame, 154848 subnormal, 77424 finite rays, 71237 ended at the end cell
    "axis_near_axis_mixed": dict(dir_untame=110_000, dir_subnormal=75_000, finite_rays=38_000, end_last_cell=35_000, end_hit=27_000),
    # 3504174 zero-axis steps, 19816 NaN heads
    "axis_untame_far": dict(zero_axis_steps=1_700_000, head_nan=9_500, dir_neg_zero=17_000),
    # 1581441 zero-axis steps, 22890 NaN heads
    "axis_untame_tiny": dict(zero_axis_steps=750_000, head_nan=11_000, dir_neg_zero=17_000),
    # 2509297 zero-axis steps, 19816 NaN heads
    "axis_untame_scaled": dict(zero_axis_steps=1_200_000, head_nan=9_500, dir_neg_zero=17_000),
    # 1660757 zero-axis steps, 22890 NaN heads
    "axis_tame_bounds": dict(zero_axis_steps=800_000, head_nan=11_000, dir_neg_zero=17_000),
    # 89150 finite rays, 10237 ended at the end cell, 12771 +0 components and NaN heads (on the planes of the lights)
    "axis_point_lights": dict(finite_rays=44_000, end_last_cell=5_000, dir_pos_zero=6_000, head_nan=6_000, origin_on_plane=45_000),
    # 9066924 zero-axis steps, 48872 hits, 109785 -0
    "axis_mirror_glass": dict(zero_axis_steps=4_500_000, end_hit=24_000, dir_neg_zero=55_000, head_nan=35_000),
    # 49477 -0, 4221314 zero-axis steps
    "axis_class_sun": dict(dir_neg_zero=24_000, zero_axis_steps=2_000_000, head_nan=14_000, bind_zero_outside=350),
})

FUZZ_SEEDS = (1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def axis_scene(name):
    return SC.axis_by_name(name)()


@pytest.fixture(scope="module")
def stored():
    z = np.load(os.path.join(GOLDEN, "ref_axis_scenes.npz"))
    return {k: z[k] for k in z.files}


def _assert_planes(got, want, what):
    for ch, g, w in zip("RGB", got, want):
        bad = int((np.asarray(g) != np.asarray(w)).sum())
        assert bad == 0, f"{what}: plane {ch} differs in {bad}/{np.asarray(w).size} pixels"


def test_every_axis_scene_has_floors():
    assert sorted(FLOORS) == sorted(AXIS_NAMES)
    assert sorted(k[:-2] for k in np.load(os.path.join(GOLDEN, "ref_axis_scenes.npz")).files if k.endswith("_r")) == sorted(AXIS_NAMES)


@pytest.mark.parametrize("name", AXIS_NAMES)
def test_axis_scene_meets_its_edge_and_matches_the_reference(name, stored):
    sc = axis_scene(name)
    planes, census = O.oracle_census(sc, THREADS)
    low = {k: (census[k], floor) for k, floor in FLOORS[name].items() if census[k] < floor}
    assert not low, f"{name}: census below its floors (value, floor): {low}; census {census}"
    assert census["end_left_grid"] + census["end_last_cell"] + census["end_hit"] == census["grid_rays"], census
    want = [stored[f"{name}_{c}"] for c in "rgb"]
    _assert_planes(planes, want, f"{name}: oracle (census) vs the stored reference planes")
    _assert_planes(O.oracle_render(sc, THREADS), want, f"{name}: oracle vs the stored reference planes")
    assert (want[0] > 0).mean() > 0.5, f"{name}: frame is mostly black"
    if O.have_ref():
        _assert_planes(O.ref_render(sc), want, f"{name}: reference kernel vs its stored planes")


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_axis_fuzz_scene_oracle_census_and_reference(seed):
    sc = SC.axis_fuzz_scene(seed)
    planes, census = O.oracle_census(sc, THREADS)
    assert census["grid_rays"] > 0 and census["dir_pos_zero"] + census["dir_untame"] > 0, (SC.axis_fuzz_summary(sc), census)
    _assert_planes(planes, O.oracle_render(sc, THREADS), f"fuzz {SC.axis_fuzz_summary(sc)}: census vs plain render")
    if O.have_ref():
        _assert_planes(planes, O.ref_render(sc), f"fuzz {SC.axis_fuzz_summary(sc)}: oracle vs the reference kernel")


def test_axis_fuzz_scenes_are_drawn_from_the_seed_alone():
    a, b = SC.axis_fuzz_scene(7), SC.axis_fuzz_scene(7)
    for k in ("vertex", "tri_index", "light_type", "light_dir", "light_pos", "light_radius", "box_min", "grid_list", "cam_list"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert SC.axis_fuzz_scene(8).vertex.tobytes() != a.vertex.tobytes() or SC.axis_fuzz_scene(8).light_dir.tobytes() != a.light_dir.tobytes()


def test_planes_tame_follows_the_hosts_rule():
    """scenarios.planes_tame is rt_api.cpp's rule: every plane coordinate 0 or 2^-60 <= |x| <= 2^39."""
    def planes(v):
        b = np.zeros((257, 4), np.float32)
        b[5, 1] = v
        return b
    for v, tame in ((0.0, True), (-0.0, True), (2.0 ** -60, True), (-(2.0 ** 39), True), (1.0, True), (2.0 ** 39, True),
                    (np.nextafter(np.float32(2.0 ** -60), np.float32(0)), False), (np.nextafter(np.float32(2.0 ** 39), np.float32(np.inf)), False),
                    (1e-40, False), (np.inf, False), (np.nan, False)):
        assert SC.planes_tame(planes(v)) == tame, v



def test_bind_in_cube_with_zero_components():
    """BindInCube (:265-322) with the point beyond one face and the direction's component on that axis +0 or -0: the '<= 0' / '0 <='
    tests return false before any clamp, so the point stays where it is (a '< 0' would divide by zero and move it to inf / NaN).
    Checked against the reference kernel where it was built."""
    lo, hi = np.array(SC.ROOM_LO, np.float32), np.array(SC.ROOM_HI, np.float32)
    inside = ((lo + hi) / 2).astype(np.float32)
    fp = lambda v: np.ascontiguousarray(v, np.float32).ctypes.data_as(O.C.POINTER(O.C.c_float))
    cases = 0
    for axis in range(3):
        for beyond in (lo[axis] - np.float32(0.5), hi[axis] + np.float32(0.5)):
            for zero in (0.0, -0.0):
                for other in ((1.0, -1.0), (0.0, 0.25), (-0.75, -0.0)):
                    p = inside.copy()
                    p[axis] = beyond
                    d = np.zeros(3, np.float32)
                    d[axis] = zero
                    d[[a for a in range(3) if a != axis]] = other
                    q = p.copy()
                    ok = O.oracle().rt_oracle_bind_in_cube(fp(q), fp(d), fp(lo), fp(hi))
                    assert ok == 0 and q.tobytes() == p.tobytes(), (axis, p, d, q)
                    if O.have_ref():
                        r = O.Float3()
                        for i in range(3):
                            r.s[i] = float(p[i])
                        assert O.ref().BindInCube(O.C.byref(r), _f3(d), _f3(lo), _f3(hi)) == 0
                        assert np.array(r.s[:3], np.float32).tobytes() == p.tobytes()
                    cases += 1
    assert cases == 36


def _f3(v):
    out = O.Float3()
    for i in range(3):
        out.s[i] = float(v[i])
    return out
