"""CPU tests: the oracle (C restatement) against the golden fixtures minted from the reference kernel, against the
function-level known answers, and against the reference kernel's stored planes of seeded random scenes (where
oracle/_ref exists, against the reference kernel itself as well)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import scenarios
from conftest import GOLDEN, golden_names, load_golden_scene


@pytest.mark.parametrize("name", golden_names())
def test_oracle_matches_golden_planes(name):
    sc, want = load_golden_scene(name)
    got = O.oracle_render(sc, threads=1)
    for ch, g, w in zip("RGB", got, want):
        assert np.array_equal(g, w), f"{name}: plane {ch} differs in {(g != w).sum()} pixels"


def test_oracle_threads_do_not_change_planes():
    sc, want = load_golden_scene("sparse_many_samples")
    got = O.oracle_render(sc, threads=4)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_oracle_pixel_ranges_compose():
    sc, want = load_golden_scene("lambert_distant")
    half = sc.pixels // 2
    a = O.oracle_render(sc, first_pixel=0, pixel_count=half)
    b = O.oracle_render(sc, first_pixel=half, pixel_count=sc.pixels - half)
    for x, y, w in zip(a, b, want):
        assert np.array_equal(x + y, w)


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "kat.npz"))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_kat_randf(kat):
    L = O.oracle()
    for i, seed in enumerate(kat["rand_seeds"]):
        st = C.c_uint64(int(seed))
        for j in range(16):
            lo, hi = ((0.0, 1.0), (-1.0, 1.0))[j & 1]
            v = np.float32(L.rt_oracle_randf(C.byref(st), lo, hi))
            assert v.tobytes() == kat["rand_draws"][i, j].tobytes()
            assert st.value == int(kat["rand_states"][i, j])


def test_kat_sphere_point(kat):
    L = O.oracle()
    for i in range(len(kat["sphere_seeds"])):
        st = C.c_uint64(int(kat["sphere_seeds"][i]))
        out = np.zeros(3, np.float32)
        L.rt_oracle_sphere_point(C.byref(st), float(kat["sphere_radius"][i]), _fp(out))
        assert out.tobytes() == kat["sphere_out"][i].tobytes()
        assert st.value == int(kat["sphere_state"][i])


def test_kat_positive_modf(kat):
    L = O.oracle()
    got = np.array([L.rt_oracle_positive_modf(float(v)) for v in kat["pmodf_in"]], np.float32)
    assert got.tobytes() == kat["pmodf_out"].tobytes()
    assert np.float32(L.rt_oracle_positive_modf(-2.0 ** -30)) == np.float32(1.0)  # the 53-bit sum matters


def test_kat_ray_triangle_and_point_line(kat):
    L = O.oracle()
    n = len(kat["tri_o"])
    for i in range(n):
        t, l1, l2 = C.c_float(0), C.c_float(0), C.c_float(0)
        arrs = [np.ascontiguousarray(kat[k][i]) for k in ("tri_o", "tri_d", "tri_a", "tri_b", "tri_c")]
        hit = L.rt_oracle_ray_triangle(_fp(arrs[0]), _fp(arrs[1]), float(kat["tri_tmin"][i]), float(kat["tri_tmax"][i]),
                                       _fp(arrs[2]), _fp(arrs[3]), _fp(arrs[4]), C.byref(t), C.byref(l1), C.byref(l2))
        got = np.array([hit, t.value, l1.value, l2.value], np.float32)
        assert got.tobytes() == kat["tri_res"][i].tobytes(), i
        pl = np.float32(L.rt_oracle_point_line_sq(_fp(arrs[2]), _fp(arrs[3]), _fp(arrs[0])))
        assert pl.tobytes() == kat["pline_out"][i].tobytes(), i


def test_kat_box_address_and_bind(kat):
    L = O.oracle()
    box = np.ascontiguousarray(kat["box_min"])
    for i, p in enumerate(kat["box_pts"]):
        out = (C.c_int * 3)()
        pp = np.ascontiguousarray(p)
        L.rt_oracle_box_address(256, box.ctypes.data_as(C.c_void_p), _fp(pp), out)
        assert list(out) == list(kat["box_addr"][i]), i
    lo, hi = np.ascontiguousarray(box[0, :3]), np.ascontiguousarray(box[256, :3])
    for i in range(len(kat["bind_o"])):
        p = np.ascontiguousarray(kat["bind_o"][i]).copy()
        d = np.ascontiguousarray(kat["bind_d"][i])
        ok = L.rt_oracle_bind_in_cube(_fp(p), _fp(d), _fp(lo), _fp(hi))
        got = np.array([ok, *p], np.float32)
        assert got.tobytes() == kat["bind_res"][i].tobytes(), i


@pytest.mark.parametrize("seed", scenarios.FRESH_SEEDS)
def test_oracle_matches_reference_kernel_on_fresh_scenes(seed):
    """Seeded random scenes, not the curated ones: restatement == reference kernel, plane for plane.  The reference's planes
    are stored (tests/golden/ref_fresh_scenes.npz, minted by make_golden.py); where oracle/_ref exists the reference kernel
    is run as well and must still give the stored planes."""
    from opencl_render_amd import raytrace as R
    sc = scenarios.fresh_soup(seed)
    R.build_lists(sc)
    stored = np.load(os.path.join(GOLDEN, "ref_fresh_scenes.npz"))
    want = [stored[f"{seed}_{c}"] for c in "rgb"]
    a = O.oracle_render(sc)
    for ch, x, y in zip("RGB", a, want):
        assert np.array_equal(x, y), f"seed {seed}: plane {ch} differs from the reference's in {(x != y).sum()} pixels"
    if O.have_ref():
        for ch, x, y in zip("RGB", O.ref_render(sc), want):
            assert np.array_equal(x, y), f"seed {seed}: the reference kernel no longer gives the stored plane {ch}"


@pytest.mark.parametrize("name", [f.__name__ for f in scenarios.CLASS])
def test_oracle_matches_reference_kernel_on_class_scenes(name):
    """The opaque-diffuse scenarios (scenarios.CLASS): restatement == the reference's stored planes
    (tests/golden/ref_class_scenes.npz); where oracle/_ref exists the reference kernel must still give them."""
    from opencl_render_amd import raytrace as R
    sc = scenarios.class_by_name(name)()
    R.build_lists(sc)
    stored = np.load(os.path.join(GOLDEN, "ref_class_scenes.npz"))
    want = [stored[f"{name}_{c}"] for c in "rgb"]
    for ch, x, y in zip("RGB", O.oracle_render(sc), want):
        assert np.array_equal(x, y), f"{name}: plane {ch} differs from the reference's in {(x != y).sum()} pixels"
    if O.have_ref():
        for ch, x, y in zip("RGB", O.ref_render(sc), want):
            assert np.array_equal(x, y), f"{name}: the reference kernel no longer gives the stored plane {ch}"
    assert set(stored.files) == {f"{f.__name__}_{c}" for f in scenarios.CLASS for c in "rgb"}
