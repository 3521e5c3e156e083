"""rtHipSceneSetLights / rtHipSceneSetMaterials on the device: a resident scene whose lights, material tables or material ids were edited
is the scene a fresh upload of the edited description would have made.

The yardstick is always a FRESH ResidentScene of the edited description (the "twin": a copy of the base Scene with fields replaced through
scene.pack_lights / scene.pack_materials) -- a path the rest of the suite pins to the oracle.  Every test needs the entry points of this
feature, so all of them fail without it.  Where a test could pass on nothing (an edit that changes no pixel), it asserts that the twins of
consecutive steps differ."""
import ctypes as C

import torch  # (before the library loads its HIP runtime: the order bench.py uses)
import numpy as np
import pytest

import camera_cases as CC
import scenarios
from edit_cases import ONE_SUN, SPOT, fold, lights_of, many_lights, materials_of, twin_of
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu

WF, MEGA = R.PIPELINE_WAVEFRONT, R.PIPELINE_MEGAKERNEL
REJECTED = "a triangle uses a material >= materialCount"


@pytest.fixture(autouse=True)
def fresh_tuning():
    R.tune("reset", 0)
    yield
    R.tune("reset", 0)


_bases = {}


def base(name):
    """A scenario with the host builders' lists, made once (twins are shallow copies: nobody writes into its arrays)."""
    if name not in _bases:
        sc = getattr(scenarios, name)()
        R.build_lists(sc)
        _bases[name] = sc
    return _bases[name]


def frame(rs):
    rs.render()
    return [np.asarray(p).copy() for p in rs.readback()]


def fresh(sc, pipeline=WF, window=None, tiles=None):
    """The planes of a scene created fresh from `sc`."""
    rs = R.ResidentScene(sc, 0, tiles)
    try:
        rs.set_pipeline(pipeline)
        if window:
            rs.set_sample_window(**window)
        return frame(rs)
    finally:
        rs.close()


def assert_planes(got, want, label):
    for ch, g, w in zip("RGB", got, want):
        bad = np.nonzero(np.asarray(g).reshape(-1) != np.asarray(w).reshape(-1))[0]
        assert bad.size == 0, f"{label}: plane {ch} differs in {bad.size} pixels, first {bad[:5]}"


def differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def rows(rs):
    return np.asarray(rs.scene_view("tri_shade")).reshape(-1, 24).view(np.int32).copy()


LIGHT_STEPS = [("none", lambda: []), ("one_distant", lambda: ONE_SUN), ("spot_finite_range", scenarios.spot_finite_range),
               ("all_light_types", scenarios.all_light_types), ("64", lambda: many_lights(64, 1)), ("65", lambda: many_lights(65, 2)),
               ("70", lambda: many_lights(70, 3)), ("back_to_one", lambda: ONE_SUN)]
LIGHT_COUNTS = [0, 1, 2, 11, 64, 65, 70, 1]


@pytest.fixture(scope="module")
def hall():
    """mirror_hall resident for the steps of test_lights_general_class, which run in order on this one scene, and its first frame."""
    sc = base("mirror_hall")
    rs = R.ResidentScene(sc, 0)
    try:
        yield sc, rs, frame(rs)
    finally:
        rs.close()


@pytest.mark.parametrize("step", range(len(LIGHT_STEPS)), ids=[s[0] for s in LIGHT_STEPS])
def test_lights_general_class(hall, step):
    """1: mirror_hall through light sets of 0, 1, 2, 11, 64, 65, 70 and 1 lights in this order on ONE resident scene (both sides of the
    logic kernel's 64-light split; a step is checked against the twin of its own light set, so it does not need the steps before it to
    have run): after the edit the watched frame and the planned frame after it equal the twin's; on the 0-, 1-, 2- and 65-light steps
    the megakernel's frame does too."""
    sc, rs, first = hall
    label, make = LIGHT_STEPS[step]
    spec = make()
    L = lights_of(spec)
    assert L["light_type"].shape[0] == LIGHT_COUNTS[step]
    twin = twin_of(sc, lights=L)
    want = fresh(twin)
    assert differ(want, first), f"{label}: the twin's frame equals the frame under the scene's own lights"
    rs.set_lights(spec if isinstance(spec, list) else L)
    assert rs.path_class() == R.path_class(twin) == R.PATH_CLASS_GENERAL
    assert_planes(frame(rs), want, f"{label}: watched frame")
    assert_planes(frame(rs), want, f"{label}: planned frame")
    assert rs.finish() is False, f"{label}: the planned frame had to be redone"
    if LIGHT_COUNTS[step] in (0, 1, 2, 65) and step < 7:
        rs.set_pipeline(MEGA)
        assert_planes(frame(rs), fresh(twin, MEGA), f"{label}: megakernel")
        rs.set_pipeline(WF)
    for k in R.LIGHT_FIELDS:
        assert np.asarray(getattr(rs.scene, k)).tobytes() == np.asarray(L[k]).tobytes(), k
    assert rs.edit_times_ms()["lights"] > 0 and rs.edit_times_ms()["materials"] == 0


def test_lights_class_transitions_keep_the_sample_window():
    """2: lambert_distant through 1 -> 2 -> 1 -> 0 lights under a non-default sample window: path class and frames follow the twin, and
    the window -- next and last -- is what it was before the edit that crosses the one / several boundary."""
    sc = base("lambert_distant")
    window = dict(total=4, first=2, divisor=2, accumulate=False)
    one = lights_of(sc)
    steps = [("two", lights_of(ONE_SUN + [SPOT]), R.PATH_CLASS_GENERAL), ("one", one, R.PATH_CLASS_OPAQUE_DIFFUSE),
             ("none", lights_of([]), R.PATH_CLASS_OPAQUE_DIFFUSE)]
    rs = R.ResidentScene(sc, 0)
    try:
        assert rs.path_class() == R.PATH_CLASS_OPAQUE_DIFFUSE
        rs.set_sample_window(**window)
        before = frame(rs)
        assert_planes(before, fresh(sc, window=window), "base under the window")
        assert differ(before, fresh(sc)), "the window draws the default window's samples"
        for label, L, cls in steps:
            held = rs.sample_window()
            assert held["next"]["first"] == 2 and held["last"]["total"] == 4
            twin = twin_of(sc, lights=L)
            rs.set_lights(L)
            assert rs.sample_window() == held, f"{label}: the edit moved the sample window"
            assert rs.path_class() == R.path_class(twin) == cls, label
            want = fresh(twin, window=window)
            assert differ(want, before), label
            assert_planes(frame(rs), want, f"{label}: watched frame")
            assert_planes(frame(rs), want, f"{label}: planned frame")
            before = want
    finally:
        rs.close()


def test_materials_class_transitions():
    """2b: lambert_distant (one light) from the opaque-diffuse class to the general one by mirror_hall's reflective and transparent
    materials, and back by one Lambert material."""
    sc = base("lambert_distant")
    hall = materials_of(scenarios.mirror_hall())
    ids = (np.arange(sc.triangle_count) % 4).astype(np.int32)
    white = materials_of([scenarios._lambert(color=(250, 240, 230))])
    rs = R.ResidentScene(sc, 0)
    try:
        assert rs.path_class() == R.PATH_CLASS_OPAQUE_DIFFUSE
        before = frame(rs)
        for label, mats, new_ids, cls in (("mirrors", hall, ids, R.PATH_CLASS_GENERAL), ("lambert", white, fold(ids, 1), R.PATH_CLASS_OPAQUE_DIFFUSE)):
            twin = twin_of(sc, materials=mats, ids=new_ids)
            rs.set_materials(mats, new_ids)
            assert rs.path_class() == R.path_class(twin) == cls, label
            want = fresh(twin)
            assert differ(want, before), label
            assert_planes(frame(rs), want, f"{label}: watched frame")
            assert_planes(frame(rs), want, f"{label}: planned frame")
            before = want
    finally:
        rs.close()


def surface(rs):
    planes = frame(rs)
    p = rs.readback_passes()
    return planes, p["normal"].copy(), p["albedo"].copy()


def test_materials_tables_ids_and_the_refused_shrink():
    """3: mixed_materials_textured with the normal and albedo passes on: mirror_hall's four materials with ids folded into range; a
    shrink to two materials WITHOUT ids is refused (-5) and changes nothing; the same with ids succeeds; then one Lambert material.
    Frames, normal and albedo equal the twin's."""
    sc = base("mixed_materials_textured")
    hall = scenarios.mirror_hall()
    four = materials_of(hall)
    two = dict(mat_size=hall.mat_size[:10].copy(), mat_start=hall.mat_start[:11].copy(), textures=hall.textures)
    lambert = materials_of([scenarios._lambert(color=(200, 220, 255))])

    def twin_surface(twin):
        rs = R.ResidentScene(twin, 0)
        try:
            rs.set_passes(normal=True, albedo=True)
            return surface(rs)
        finally:
            rs.close()

    def check(rs, twin, label):
        want = twin_surface(twin)
        got = surface(rs)
        assert_planes(got[0], want[0], label)
        assert got[1].tobytes() == want[1].tobytes(), f"{label}: normal pass"
        assert got[2].tobytes() == want[2].tobytes(), f"{label}: albedo pass"
        assert rs.path_class() == R.path_class(twin), label
        return want

    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(normal=True, albedo=True)
        base_surface = surface(rs)
        ids4 = fold(sc.tri_material, 4)
        assert ids4.max() == 3 and ids4.min() == -1
        rs.set_materials(four, ids4)
        first = check(rs, twin_of(sc, materials=four, ids=ids4), "four materials")
        assert differ(first[0], base_surface[0]) and first[2].tobytes() != base_surface[2].tobytes()
        assert rs.edit_times_ms()["materials"] > 0 and rs.edit_times_ms()["ids"] > 0
        held, pointers = surface(rs), rs.pointers()
        assert rs.try_set_materials(two) == -5, R.last_error()
        assert "scene rejected" in R.last_error() and REJECTED in R.last_error(), R.last_error()
        assert rs.pointers() == pointers and rs.scene.material_count == 4
        again = surface(rs)
        assert_planes(again[0], held[0], "after the refused shrink")
        assert again[1].tobytes() == held[1].tobytes() and again[2].tobytes() == held[2].tobytes()
        ids2 = fold(sc.tri_material, 2)
        assert rs.try_set_materials(two, ids2) == 0, R.last_error()
        assert rs.pointers()[4] != 0 and rs.scene.material_count == 2
        second = check(rs, twin_of(sc, materials=two, ids=ids2), "two materials")
        assert differ(second[0], first[0])
        ids1 = fold(sc.tri_material, 1)
        rs.set_materials(lambert, ids1)
        check(rs, twin_of(sc, materials=lambert, ids=ids1), "one Lambert material")
        # tables alone, ids kept: every resident id is 0 or -1, so any table of one material or more is legal
        rs.set_materials(four)
        check(rs, twin_of(sc, materials=four, ids=ids1), "tables alone")
    finally:
        rs.close()


TWO_COLOURS = [scenarios._lambert(), scenarios._lambert(color=(220, 40, 30))]


@pytest.mark.parametrize("T", [1, 63, 64, 65, 256, 257])
def test_ids_only_wave_and_workgroup_tails(T):
    """4: a soup of T triangles, two materials: a permuted id array with some -1 as numpy and another as a torch tensor -- word 21 of every
    row is the id, the other 23 words keep their bits, the frame is the twin's; an array whose only bad id sits at triangle 0, or at
    triangle T - 1, is refused with rows and frame unchanged."""
    rng = np.random.Generator(np.random.PCG64(1000 + T))
    sc = S.make_soup(24, 16, T, 0.5, seed=500 + T, samples=1, materials=TWO_COLOURS, material_ids=(np.arange(T) % 2).astype(np.int32))
    R.build_lists(sc)
    first_ids = np.where(rng.random(T) < 0.2, -1, rng.permutation(np.arange(T) % 2)).astype(np.int32)
    if T == 1:
        first_ids[:] = 1
    second_ids = np.where(first_ids < 0, 0, np.where(np.arange(T) % 3 == 0, -1, 1 - first_ids)).astype(np.int32)
    rs = R.ResidentScene(sc, 0)
    try:
        before = rows(rs)
        assert np.array_equal(before[:, 21], sc.tri_material)
        for label, ids, give in (("numpy", first_ids, lambda a: a), ("torch", second_ids, lambda a: torch.from_numpy(a).to(torch.device("cuda", 0)))):
            assert not np.array_equal(ids, before[:, 21]), label
            rs.set_materials(tri_material=give(ids))
            now = rows(rs)
            assert np.array_equal(now[:, 21], ids), f"{label}: word 21"
            assert np.array_equal(np.delete(now, 21, axis=1), np.delete(before, 21, axis=1)), f"{label}: another word of a row changed"
            assert_planes(frame(rs), fresh(twin_of(sc, ids=ids)), f"{label}: T = {T}")
            assert np.array_equal(np.asarray(rs.scene.tri_material), ids)
            assert rs.edit_times_ms()["materials"] == 0 and rs.edit_times_ms()["ids"] > 0
            before = now
        held = frame(rs)
        for at in sorted({0, T - 1}):
            bad = second_ids.copy()
            bad[at] = 2
            for give in (lambda a: a, lambda a: torch.from_numpy(a).to(torch.device("cuda", 0))):
                assert rs.try_set_materials(tri_material=give(bad)) == -5, (at, R.last_error())
                assert "scene rejected" in R.last_error() and REJECTED in R.last_error()
                assert np.array_equal(rows(rs), before), f"bad id at triangle {at}: rows changed"
            assert_planes(frame(rs), held, f"bad id at triangle {at}")
        assert np.array_equal(np.asarray(rs.scene.tri_material), second_ids)
    finally:
        rs.close()


def scaled(sc, f):
    v = sc.vertex.copy()
    v[:, :3] = (v[:, :3].astype(np.float64) * np.array(f)).astype(np.float32)
    return v


def shaped(sc, vertex):
    out = twin_of(sc, vertex=vertex)
    out.box_min = out.grid_start = out.grid_list = out.cam_start = out.cam_end = out.cam_list = None
    R.build_lists(out)
    return out


def test_with_geometry_updates_both_triangle_sets():
    """5a, 5b: ids, then set_vertices: the ids are carried into the second triShade set; set_vertices, then ids -- twice, so that each of
    the two sets has been the one in use -- : the store hits the set the frames read."""
    sc = base("mixed_materials_textured")
    T, M = sc.triangle_count, sc.material_count
    ids_a = ((np.arange(T) * 7) % M).astype(np.int32)
    ids_b = np.where(np.arange(T) % 5 == 0, -1, (np.arange(T) * 3 + 1) % M).astype(np.int32)
    ids_c = ((np.arange(T) // 3) % M).astype(np.int32)
    big, tall = shaped(sc, scaled(sc, (1.25, 0.8, 1.1))), shaped(sc, scaled(sc, (0.9, 1.3, 1.0)))
    rs = R.ResidentScene(sc, 0)
    try:
        frame(rs)
        rs.set_materials(tri_material=ids_a)
        rs.set_vertices(big.vertex, sc.tri_index)
        assert np.array_equal(rows(rs)[:, 21], ids_a)
        assert_planes(frame(rs), fresh(twin_of(big, ids=ids_a)), "ids, then vertices")
        first_set = rs.pointers()[1]
        rs.set_materials(tri_material=ids_b)  # the scene reads the first spare set now
        assert rs.pointers()[1] == first_set and np.array_equal(rows(rs)[:, 21], ids_b)
        want_b = fresh(twin_of(big, ids=ids_b))
        assert differ(want_b, fresh(twin_of(big, ids=ids_a)))
        assert_planes(frame(rs), want_b, "vertices, then ids")
        rs.set_vertices(tall.vertex)  # ... and now the other one
        assert rs.pointers()[1] != first_set
        rs.set_materials(tri_material=ids_c)
        assert np.array_equal(rows(rs)[:, 21], ids_c)
        assert_planes(frame(rs), fresh(twin_of(tall, ids=ids_c)), "vertices again, then ids")
        rs.set_vertices(big.vertex)  # back in the first set: the ids come over from the rows that were edited last
        assert rs.pointers()[1] == first_set and np.array_equal(rows(rs)[:, 21], ids_c)
        assert_planes(frame(rs), fresh(twin_of(big, ids=ids_c)), "ids carried back")
    finally:
        rs.close()


def test_with_a_camera_move_and_the_bake_filter():
    """5c, 5d: set_lights, then set_camera; the AO bake's `material` filter after a reassignment selects the twin's triangles."""
    sc = base("mixed_materials_textured")
    T, M = sc.triangle_count, sc.material_count
    L = lights_of(ONE_SUN + [SPOT])
    pan = CC.posed(sc, "pan", lists=False)
    twin = twin_of(pan, lights=L)
    twin.cam_start = twin.cam_end = twin.cam_list = None
    R.build_camera_list(twin)
    ids = ((np.arange(T) * 11 + 2) % M).astype(np.int32)
    rs = R.ResidentScene(sc, 0)
    try:
        frame(rs)
        rs.set_lights(L)
        rs.set_camera(pan.eye, pan.eye_to_top_left, pan.left_to_right, pan.top_to_bottom, pan.pixel_size_inv)
        assert_planes(frame(rs), fresh(twin), "lights, then camera")
        rs.set_materials(tri_material=ids)
        got = rs.bake_ambient_occlusion(64, 64, rays=4, material=2)
    finally:
        rs.close()
    fr = R.ResidentScene(twin_of(sc, ids=ids), 0)
    try:
        want = fr.bake_ambient_occlusion(64, 64, rays=4, material=2)
    finally:
        fr.close()
    old = R.ResidentScene(sc, 0)
    try:
        stale = old.bake_ambient_occlusion(64, 64, rays=4, material=2)
    finally:
        old.close()
    assert got["ao"].tobytes() == want["ao"].tobytes() and got["triangle"].tobytes() == want["triangle"].tobytes()
    covered = want["triangle"][want["triangle"] != 0xFFFFFFFF]
    assert covered.size > 0 and (ids[covered] == 2).all()
    assert stale["triangle"].tobytes() != want["triangle"].tobytes()  # the filter read the new ids


def test_tile_subsets_and_peers():
    """6: two instances over a disjoint deal of odd_size_multi_tile's four tiles, the second made like the first, both edited: the
    composed image is the twin's; an instance made like an edited scene, from the edited scene's own description, renders it too."""
    sc = base("odd_size_multi_tile")
    L = lights_of(ONE_SUN + [dict(type=S.LIGHT_AREA, pos=(-0.8, -0.3, 2.5), col=(0.3, 0.5, 0.9), radius=0.05, half_att=0.75)])
    mats = materials_of(TWO_COLOURS + [scenarios._lambert(color=scenarios._tex(5, 6))])
    ids = (np.arange(sc.triangle_count) % 3).astype(np.int32)
    twin = twin_of(sc, lights=L, materials=mats, ids=ids)
    want = fresh(twin)
    assert differ(want, fresh(sc))
    a = R.ResidentScene(sc, 0, tiles=R.tiles_of_rank(sc.width, sc.height, 0, 2))
    b = R.ResidentScene(sc, 0, tiles=R.tiles_of_rank(sc.width, sc.height, 1, 2), like=a)
    c = None
    try:
        assert len(a.tiles) + len(b.tiles) == 4
        for rs in (a, b):
            rs.set_lights(L)
            rs.set_materials(mats, ids)
        out = [np.zeros((sc.height, sc.width), np.uint16) for _ in range(3)]
        for rs in (a, b):
            rs.render()
            rs.readback(out)
        assert_planes(out, want, "two edited instances")
        c = R.ResidentScene(a.scene, 0, like=a)
        assert c.path_class() == R.path_class(twin)
        assert_planes(frame(c), want, "an instance made like an edited scene")
    finally:
        for rs in (a, b, c):
            if rs is not None:
                rs.close()


def test_a_clone_of_a_scene_grown_to_two_lights_outlives_its_source():
    """6b: class_degenerate_outside (one light) gets a second light by an edit -- a lights part built beside the old one and installed,
    and path state for several lights handed to the path-state part -- and is then the `like` of a new instance.  The source is destroyed
    before the clone renders: the clone's blocks are its own, and its frame and its bytes are those of a scene created fresh with the
    two lights."""
    sc = base("class_degenerate_outside")
    L = lights_of(ONE_SUN + [SPOT])
    fr = R.ResidentScene(twin_of(sc, lights=L), 0)
    try:
        want, want_bytes = frame(fr), fr.bytes()
    finally:
        fr.close()
    src, clone = R.ResidentScene(sc, 0), None
    try:
        assert src.path_class() == R.PATH_CLASS_OPAQUE_DIFFUSE
        before = src.bytes()
        src.set_lights(L)
        assert src.path_class() == R.PATH_CLASS_GENERAL and src.bytes() > before
        clone = R.ResidentScene(src.scene, 0, like=src)
    finally:
        src.close()
    try:
        assert_planes(frame(clone), want, "a clone of a grown scene, after its source went")
        assert clone.bytes() == want_bytes
    finally:
        clone.close()


def test_history_is_the_callers():
    """7: an edit keeps the temporal history: the accumulation after a re-lit frame still holds the old lighting; after reset_temporal it
    is, bit for bit, a fresh twin's first accumulation."""
    sc = base("lambert_distant")
    green = lights_of([dict(type=S.LIGHT_DISTANT, dir=(-0.4, -0.6, 0.5), col=(0.05, 0.95, 0.05))])
    rs = R.ResidentScene(sc, 0)
    try:
        frame(rs)
        rs.temporal(max_history=32)
        rs.set_lights(green)
        own = np.stack([p.reshape(sc.height, sc.width) for p in frame(rs)], -1)
        blended = rs.temporal(max_history=32)
        assert float(blended["count"].max()) >= 2, "the history was dropped by the edit"
        hit = blended["count"] >= 2
        assert (np.stack(blended["planes"], -1)[hit] != own[hit]).any(), "the accumulation is the re-lit frame alone"
        rs.reset_temporal()
        alone = rs.temporal(max_history=32)
    finally:
        rs.close()
    fr = R.ResidentScene(twin_of(sc, lights=green), 0)
    try:
        frame(fr)
        want = fr.temporal(max_history=32)
    finally:
        fr.close()
    assert alone["colour"].tobytes() == want["colour"].tobytes() and alone["count"].tobytes() == want["count"].tobytes()
    assert_planes(alone["planes"], want["planes"], "temporal after the reset")


def test_memory_is_steady_and_refusals_change_nothing():
    """8: the scene holds the same bytes after the 2nd and the 5th identical edit; every -1 refusal that needs a scene leaves addresses
    and the next frame as they were."""
    sc = base("mixed_materials_textured")
    L = lights_of(ONE_SUN + [SPOT])
    mats = materials_of(scenarios.mirror_hall())
    ids = fold(sc.tri_material, 4)
    rs = R.ResidentScene(sc, 0)
    try:
        frame(rs)
        held = []
        for i in range(5):
            rs.set_lights(L)
            rs.set_materials(mats, ids)
            held.append(rs.bytes())
        assert held[1] == held[4], held
        want = frame(rs)
        assert_planes(want, fresh(twin_of(sc, lights=L, materials=mats, ids=ids)), "after five identical edits")
        pointers, lib = rs.pointers(), R.lib()
        a = {k: np.ascontiguousarray(v) for k, v in L.items()}
        size, start, tex = (np.ascontiguousarray(mats[k]) for k in ("mat_size", "mat_start", "textures"))
        past = start.copy()
        past[0] = len(tex)  # channel 0 of material 0 is one texel: one past the atlas
        assert size[0, 0] == 1 and size[0, 1] == 1
        p = {k: R._ptr(v) for k, v in a.items()}
        refusals = [
            ("host pointer as device ids", lambda: lib.rtHipSceneSetMaterials(rs.handle, C.byref(R.MaterialUpdate(0, 0, None, None, 0, None, R._ptr(ids), 1))),
             "not device memory"),
            ("neither tables nor ids", lambda: lib.rtHipSceneSetMaterials(rs.handle, C.byref(R.MaterialUpdate())), "neither"),
            ("a channel past the atlas", lambda: lib.rtHipSceneSetMaterials(rs.handle, C.byref(R.MaterialUpdate(
                1, 4, R._ptr(size), R._ptr(past), len(tex), R._ptr(tex), None, 0))), "exceed"),
            ("NULL table", lambda: lib.rtHipSceneSetMaterials(rs.handle, C.byref(R.MaterialUpdate(1, 4, None, R._ptr(start), len(tex), R._ptr(tex), None, 0))),
             "null material table"),
            ("65536 lights", lambda: lib.rtHipSceneSetLights(rs.handle, C.byref(R.Lights(65536, *[p[k] for k in R.LIGHT_FIELDS]))), "too large"),
            ("NULL light array", lambda: lib.rtHipSceneSetLights(rs.handle, C.byref(R.Lights(2, p["light_type"], None, p["light_dir"], p["light_col"],
                                                                                                 p["light_radius"], p["light_half_att"]))), "null light array"),
        ]
        for label, call, text in refusals:
            assert call() == -1, (label, R.last_error())
            assert text in R.last_error(), (label, R.last_error())
            assert rs.pointers() == pointers and rs.bytes() == held[4], label
            assert_planes(frame(rs), want, f"after the refusal: {label}")
        with pytest.raises(ValueError):
            rs.set_materials(tri_material=torch.from_numpy(ids))  # a host tensor is not handed over as a device pointer
        with pytest.raises(ValueError):
            rs.set_materials(tri_material=ids[:-1])
        with pytest.raises(RuntimeError):
            rs.set_materials()
        assert_planes(frame(rs), want, "after the refused arguments")
    finally:
        rs.close()


def test_command_line_relight(tmp_path):
    """9: --relight 3 through the command line's own loop: three images, image k byte for byte what the same writer gives for a scene
    created fresh with relight(lights, k, 3)."""
    from opencl_render_amd import __main__ as cli
    argv = ["--scene", "soup", "--triangles", "400", "--width", "48", "--height", "36", "--samples", "2", "--relight", "3",
            "--out", str(tmp_path / "img.ppm")]
    assert cli.main(argv) == 0
    images = [(tmp_path / f"img_{i:03d}.ppm").read_bytes() for i in range(3)]
    assert len(set(images)) == 3  # the lightings differ
    args = cli.parse_args(argv)
    sc = S.make_soup(48, 36, 400, 0.02, samples=2)
    R.build_lists(sc)
    for k in range(3):
        planes = [p.reshape(36, 48) for p in fresh(twin_of(sc, lights=R.relight(R.scene_lights(sc), k, 3)))]
        args.out = str(tmp_path / f"fresh_{k}.ppm")
        cli.write_view(args, dict(out=args.out, passes=None, denoise=None, ao=None), planes, None, None, None)
        assert (tmp_path / f"fresh_{k}.ppm").read_bytes() == images[k], f"lighting {k}"
