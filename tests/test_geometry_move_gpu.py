"""rtHipSceneSetGeometry on the device: a resident scene whose vertices moved is the scene a fresh upload would have made.

The oracle is never the code under test: for a deformation (tests/geometry_cases.py), a copy of the Scene with the arrays replaced, the
grid of oracle_lib.oracle_scene_grid, the lists of oracle_lib.oracle_camera_list, the planes of oracle_lib.oracle_render, and
prep_oracle's restatements of the device arrays.  Every test here needs the entry points of this feature, so all of them fail without it.

Conditions that keep the tests from passing on nothing are asserted where the oracle's results are made (the `deformations` fixture)."""
import os

import torch  # (before the library loads its HIP runtime: the order bench.py uses)
import numpy as np
import pytest

import builder_cases as BC
import camera_cases as CC
import geometry_cases as GC
from geometry_checks import assert_device_arrays, update_to  # (shared with the session tests)
import oracle_lib as O
import prep_oracle as P
import scenarios
from opencl_render_amd import raytrace as R

pytestmark = pytest.mark.gpu

THREADS = min(os.cpu_count() or 1, 16)
PIPELINES = [R.PIPELINE_WAVEFRONT, R.PIPELINE_MEGAKERNEL]


@pytest.fixture(autouse=True)
def fresh_tuning():
    R.tune("reset", 0)
    yield
    R.tune("reset", 0)


def oracle_planes(sc):
    return [p.reshape(-1) for p in O.oracle_render(sc, threads=THREADS)]


def frame(rs):
    rs.render()
    return rs.readback()


def assert_planes(got, want, label):
    for ch, g, w in zip("RGB", got, want):
        bad = np.nonzero(np.asarray(g).reshape(-1) != np.asarray(w).reshape(-1))[0]
        assert bad.size == 0, f"{label}: plane {ch} differs in {bad.size} pixels, first {bad[:5]}"


def update(rs, arrays):
    rs.set_vertices(*arrays)


def base_scene(name):
    sc = getattr(scenarios, name)()
    sc.box_min, sc.grid_start, sc.grid_list = O.oracle_scene_grid(sc)
    return CC.posed(sc, "home")


_cache = {}


def deformation_set(name):
    """scene -> (base, base planes, {deformation: (arrays, oracle Scene, oracle planes)}), with the conditions asserted: every deformation
    but the re-indexing changes the oracle's planes in at least 1 % of the pixels; every one but the normals-only case (whose grid must
    stay: the grid does not read normals) and "home" changes the oracle grid; the re-indexing either moves the planes or keeps the frame."""
    if name in _cache:
        return _cache[name]
    sc = base_scene(name)
    planes0 = oracle_planes(sc)
    out, shares = {}, []
    for d in GC.SEQUENCE:
        arrays = GC.arrays(sc, d)
        want = GC.with_arrays(sc, *arrays)
        planes = planes0 if d == "home" else oracle_planes(want)
        out[d] = (arrays, want, planes)
        changed = GC.changed_share(planes, planes0)
        print(f"{name}/{d}: oracle planes change in {changed:.4f} of the pixels, grid differs {GC.grid_differs(want, sc)}, "
              f"non-empty lists {CC.share_non_empty(want):.3f}, pairs {len(want.grid_list)}")
        if d == "reindex":  # the shape is the same: either the planes moved with V (then the frame may differ) or the frame is the same
            assert not np.array_equal(want.box_min, sc.box_min) or changed == 0.0, f"{name}/{d}: same planes but another frame"
        elif d == "normals":  # (the grid clause cannot hold for it: the grid does not read the normals)
            assert changed >= GC.MIN_CHANGED, f"{name}/{d}: the oracle's planes change in {changed:.4f} of the pixels only"
            assert not GC.grid_differs(want, sc), f"{name}/{d}: normals alone moved the grid"
        elif d != "home":
            assert changed >= GC.MIN_CHANGED, f"{name}/{d}: the oracle's planes change in {changed:.4f} of the pixels only"
            assert GC.grid_differs(want, sc), f"{name}/{d}: the oracle grid's list does not change"
        if d not in ("home", "normals"):
            shares.append(CC.share_non_empty(want))
    assert sum(s >= CC.MIN_SHARE for s in shares) >= 3, f"{name}: non-empty shares {shares}"
    _cache[name] = (sc, planes0, out)
    return _cache[name]


@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("name", CC.SCENES)
def test_frames_lists_and_device_arrays_follow_the_shape(name, pipeline):
    """1: for every deformation, planes equal the oracle's as integers, per-pixel lists equal the oracle's, the device arrays equal
    prep_oracle's for the oracle grid; the last update hands the original arrays back and gives the first frame again."""
    sc, planes0, cases = deformation_set(name)
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_pipeline(pipeline)
        first = frame(rs)
        assert_planes(first, planes0, f"{name}: first frame")
        bytes0 = rs.bytes()
        nulls = [0, 0]
        for d in GC.SEQUENCE:
            arrays, want, planes = cases[d]
            no_idx, no_nrm = update_to(rs, want)
            nulls[0] += no_idx; nulls[1] += no_nrm
            label = f"{name}/{d}, pipeline {pipeline}"
            CC.assert_lists_equal(rs, want, label)
            assert_device_arrays(rs, want, label)
            log = rs.geometry_log()
            assert log["pairs"] == len(want.grid_list) and log["thread"] + log["group"] == sc.triangle_count, (label, log)
            assert_planes(frame(rs), planes, label)
            assert rs.scene.vertex.tobytes() == want.vertex.tobytes() and rs.scene.tri_index.tobytes() == want.tri_index.tobytes()
        assert_planes(frame(rs), first, f"{name}: back at the original arrays")
        assert nulls[0] >= 2 and nulls[1] >= 4, nulls  # updates without an index array, without normals
        assert rs.bytes() > bytes0  # the spare set and the build scratch are counted
    finally:
        rs.close()


def test_normals_alone_change_the_normal_pass():
    """The normals-only deformation changes the NORMAL pass of the oracle-side restatement of test_surface_passes_gpu.py (a sample of the
    pixels), and the updated scene's surface passes equal a fresh scene's."""
    import test_surface_passes_gpu as SP
    sc, _, cases = deformation_set("lambert_distant")
    arrays, want, _ = cases["normals"]
    pixels = np.arange(0, sc.pixels, 53)
    before, _ = SP.surface_definition(sc, pixels)
    after, seen = SP.surface_definition(want, pixels)
    assert seen["hit_samples"] > 0 and not np.array_equal(before["normal"], after["normal"])
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(normal=True, albedo=True)
        update_to(rs, want)
        frame(rs)
        got = rs.readback_passes()
        flat = got["normal"].reshape(-1, 3)[pixels]
        assert np.array_equal(flat.view(np.uint32), after["normal"].reshape(-1, 3)[pixels].view(np.uint32))
    finally:
        rs.close()


def scaled(sc, f=(1.25, 0.8, 1.1)):
    v = sc.vertex.copy()
    v[:, :3] = (v[:, :3].astype(np.float64) * np.array(f)).astype(np.float32)
    return v


def test_both_fill_paths_over_the_builder_families():
    """2: every family of tests/builder_cases.py, created, updated to a scaled copy and back: lists and log follow the oracle grid; over
    the families both the per-thread and the per-workgroup fill ran; with build_key_cap low the fill runs twice and still matches."""
    threads = groups = 0
    for name in BC.NAMES:
        sc = BC.make(name)
        sc.box_min, sc.grid_start, sc.grid_list = O.oracle_scene_grid(sc)
        home = CC.posed(sc, "home")
        big = GC.with_arrays(home, scaled(home), home.tri_index)
        rs = R.ResidentScene(home, 0)
        try:
            assert rs.geometry_log() == dict(thread=0, group=0, attempts=0, pairs=0, entries=0, allocated=0)
            for want, arrays in ((big, (big.vertex, big.tri_index)), (home, (home.vertex,))):
                update(rs, arrays)
                log = rs.geometry_log()
                assert log["pairs"] == len(want.grid_list), f"family {name}: {log} against {len(want.grid_list)} oracle pairs"
                assert log["thread"] + log["group"] == sc.triangle_count and log["attempts"] == 1
                assert log["entries"] == CC.assert_lists_equal(rs, want, f"family {name}")
                assert_device_arrays(rs, want, f"family {name}")
                threads += log["thread"]; groups += log["group"]
            assert_planes(frame(rs), oracle_planes(home), f"family {name}: back home")
        finally:
            rs.close()
    assert threads > 0 and groups > 0, f"per-thread {threads}, per-workgroup {groups}: one of the two fills never ran"
    sc, planes0, cases = deformation_set("lambert_distant")
    arrays, want, planes = cases["scale"]
    rs = R.ResidentScene(sc, 0)
    try:
        R.tune("build_key_cap", 64)
        update_to(rs, want)
        assert rs.geometry_log()["attempts"] == 2 and rs.geometry_log()["pairs"] == len(want.grid_list) > 64
        assert_device_arrays(rs, want, "low key capacity")
        assert_planes(frame(rs), planes, "low key capacity")
    finally:
        rs.close()


def move(rs, sc):
    rs.set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)


@pytest.mark.parametrize("order", ["update_first", "move_first"])
def test_composition_with_the_camera_move(order):
    """3: update, move, update, move (and move, update, move, update) against the oracle at the final state."""
    sc, _, cases = deformation_set("mixed_materials_textured")
    twist, scale = (cases["twist"][0][0], sc.tri_index), (cases["scale"][0][0], sc.tri_index)
    final = GC.with_arrays(CC.posed(sc, "orbit90", lists=False), *scale)
    pan = CC.posed(sc, "pan", lists=False)
    rs = R.ResidentScene(sc, 0)
    try:
        frame(rs)
        steps = [("u", twist), ("m", pan), ("u", scale), ("m", final)] if order == "update_first" else [("m", pan), ("u", twist), ("m", final), ("u", scale)]
        for kind, arg in steps:
            update(rs, arg) if kind == "u" else move(rs, arg)
        CC.assert_lists_equal(rs, final, order)
        assert_device_arrays(rs, final, order)
        assert_planes(frame(rs), oracle_planes(final), order)
    finally:
        rs.close()


def test_everything_else_follows():
    """4: with all five passes on, passes, surface passes, denoise, AO image, AO bake and ray queries of an updated scene equal a
    scene's created fresh from the same arrays, bit for bit."""
    sc, _, cases = deformation_set("mixed_materials_textured")
    arrays, want, _ = cases["twist"]
    rng = np.random.default_rng(11)
    o = (rng.normal(size=(4096, 3)) * 0.5 + CC.CENTRE).astype(np.float32)
    d = rng.normal(size=(4096, 3)).astype(np.float32)

    def everything(rs):
        rs.set_passes(alpha=True, depth=True, triangle=True, normal=True, albedo=True)
        planes = frame(rs)
        out = dict(("plane%d" % i, np.asarray(p)) for i, p in enumerate(planes))
        out.update(("pass_" + k, v) for k, v in rs.readback_passes().items())
        out.update(("denoise_" + k, np.asarray(v)) for k, v in rs.denoise().items() if isinstance(v, np.ndarray))
        out["ao"] = rs.ambient_occlusion(rays=4)
        bake = rs.bake_ambient_occlusion(64, 64, rays=4)
        out.update(("bake_" + k, np.asarray(v)) for k, v in bake.items() if isinstance(v, np.ndarray))
        out.update(("hit_" + k, np.asarray(v)) for k, v in rs.intersect(o, d).items())
        return out

    fresh = R.ResidentScene(want, 0)
    try:
        exp = everything(fresh)
    finally:
        fresh.close()
    rs = R.ResidentScene(sc, 0)
    try:
        frame(rs)
        update_to(rs, want)
        got = everything(rs)
    finally:
        rs.close()
    assert set(got) == set(exp) and len(got) >= 10
    for k in exp:
        assert got[k].tobytes() == exp[k].tobytes(), f"{k} differs between the updated and the fresh scene"
    assert int((exp["hit_triangle"] != 0xFFFFFFFF).sum()) > 100 and float(exp["ao"].max()) > 0


def test_tile_subsets_and_peers():
    """5: two instances over a round-robin deal, the second made like the first, both updated: the composed planes are the oracle's."""
    sc, _, cases = deformation_set("odd_size_multi_tile")
    arrays, want, planes = cases["scale"]
    a = R.ResidentScene(sc, 0, tiles=R.tiles_of_rank(sc.width, sc.height, 0, 2))
    b = R.ResidentScene(sc, 0, tiles=R.tiles_of_rank(sc.width, sc.height, 1, 2), like=a)
    c = None
    try:
        for rs in (a, b):
            update_to(rs, want)
            CC.assert_lists_equal(rs, want, "tile subset")
        out = [np.zeros((sc.height, sc.width), np.uint16) for _ in range(3)]
        for rs in (a, b):
            rs.render()
            rs.readback(out)
        assert_planes(out, planes, "two updated instances")
        # an updated scene can be the `like` of a new instance, and its own description (lists rebuilt on the host when read) seeds it
        assert np.array_equal(a.scene.grid_list, want.grid_list) and np.array_equal(a.scene.box_min, want.box_min)
        c = R.ResidentScene(a.scene, 0, like=a)
        assert_planes(frame(c), planes, "an instance made like an updated scene")
    finally:
        for rs in (a, b, c):
            if rs is not None:
                rs.close()


def test_device_arrays_from_torch():
    """6: the same update from torch tensors on the GPU gives the same device arrays as from numpy."""
    sc, _, cases = deformation_set("lambert_distant")
    (v, _, _), want, planes = cases["twist"]
    rs = R.ResidentScene(sc, 0)
    try:
        dev = torch.device("cuda", 0)
        tv = torch.from_numpy(v[:, :3].copy()).to(dev)
        ti = torch.from_numpy(sc.tri_index).to(dev)
        rs.set_vertices(tv, ti)
        assert all(hasattr(rs.scene.__dict__[k], "data_ptr") for k in ("vertex", "tri_index"))  # the tensors were kept, not downloaded
        assert rs.scene.vertex_count == sc.vertex_count and rs.scene.triangle_count == sc.triangle_count
        assert hasattr(rs.scene.__dict__["vertex"], "data_ptr")
        assert_device_arrays(rs, want, "torch tensors")
        assert rs.scene.vertex.tobytes() == want.vertex.tobytes() and isinstance(rs.scene.__dict__["vertex"], np.ndarray)  # on first read
        CC.assert_lists_equal(rs, want, "torch tensors")
        assert_planes(frame(rs), planes, "torch tensors")
        rs.set_vertices(torch.from_numpy(sc.vertex).to(dev))  # the retained index array
        assert_planes(frame(rs), oracle_planes(sc), "torch tensors, back")
        with pytest.raises(ValueError):
            rs.set_vertices(torch.from_numpy(v))  # a host tensor is not handed over as a device pointer
    finally:
        rs.close()


def snapshot(rs):
    out = {n: rs.scene_view(n).copy() for n in ("tri_rec", "tri_shade", "grid_bits", "block_sparse", "pair_rec", "cell_lut", "cam_start", "cam_end")}
    out["cam_list"] = rs.camera_list()
    out["header"] = np.asarray(rs.scene_view("header")).copy()
    return out


def test_transactional_refusals():
    """7: each refusal leaves frame, lists and device arrays as they were, and a following valid update succeeds."""
    sc, planes0, cases = deformation_set("lambert_distant")
    arrays, want, planes = cases["scale"]
    rs = R.ResidentScene(sc, 0)
    try:
        first = frame(rs)
        assert rs.try_set_vertices(sc.vertex) == -1 and "retained" in R.last_error()  # nothing retained on a never-updated scene
        # refusals on the first-update path: the scene still renders from the parts it was created with
        created = snapshot(rs)
        wrong = sc.tri_index.copy()
        wrong[0, 0] = -1
        R.tune("build_list_limit", len(want.grid_list) - 1)
        try:
            codes = [rs.try_set_vertices(sc.vertex, wrong), rs.try_set_vertices(want.vertex, want.tri_index)]
        finally:
            R.tune("reset", 0)
        assert codes == [-5, -3], (codes, R.last_error())
        assert rs.geometry_log()["pairs"] == 0 and rs.try_set_vertices(sc.vertex) == -1  # still nothing retained
        for k, v in snapshot(rs).items():
            assert np.array_equal(created[k], v), f"first-update refusals: {k} changed"
        assert_planes(frame(rs), first, "after the first-update refusals")
        update(rs, (sc.vertex, sc.tri_index))  # from here on the scene holds its spare set and an index array
        assert_planes(frame(rs), first, "after the identity update")
        before, bytes0 = snapshot(rs), rs.bytes()
        bad = want.tri_index.copy()
        bad[sc.triangle_count // 2, 1] = sc.vertex_count
        refusals = [("index >= V", lambda: rs.try_set_vertices(want.vertex, bad), -5, P.rejection_text(P.ERR_TRI_INDEX))]

        def limited():
            R.tune("build_list_limit", len(want.grid_list) - 1)
            try:
                return rs.try_set_vertices(want.vertex)
            finally:
                R.tune("reset", 0)
        refusals.append(("list limit", limited, -3, "limit"))

        def host_pointer():
            up = R.GeometryUpdate(sc.vertex_count, R._ptr(want.vertex), None, None, 1)
            return int(R.lib().rtHipSceneSetGeometry(rs.handle, up))
        refusals.append(("host pointer as device array", host_pointer, -1, "not device memory"))
        refusals.append(("retained indices past a smaller V", lambda: rs.try_set_vertices(sc.vertex[: sc.vertex_count // 2]), -5, P.rejection_text(P.ERR_TRI_INDEX)))
        for label, call, code, text in refusals:
            assert call() == code, (label, R.last_error())
            assert text in R.last_error(), (label, R.last_error())
            after = snapshot(rs)
            for k in before:
                assert np.array_equal(before[k], after[k]), f"{label}: {k} changed"
            assert rs.bytes() == bytes0, f"{label}: the scene holds {rs.bytes()} bytes, {bytes0} before"  # every buffer exists by now
            assert_planes(frame(rs), first, f"after the refusal: {label}")
            assert rs.scene.vertex.tobytes() == sc.vertex.tobytes()
        update_to(rs, want)
        assert_planes(frame(rs), planes, "a valid update after the refusals")
    finally:
        rs.close()


def test_steady_state():
    """8: after one update, a second to a shape with no more pairs and entries allocates nothing; matRec and lightPos stay; planned
    frames after an update are verified and equal the watched one."""
    sc, planes0, cases = deformation_set("mixed_materials_textured")
    arrays, want, planes = cases["scale"]
    rs = R.ResidentScene(sc, 0)
    try:
        frame(rs)
        ptrs = rs.pointers()
        update_to(rs, want)
        assert rs.geometry_log()["allocated"] == 1
        held = rs.bytes()
        pairs, entries = rs.geometry_log()["pairs"], rs.geometry_log()["entries"]
        for again in ((want.vertex, want.tri_index), (want.vertex,), (want.vertex, None, want.tri_normal)):
            update(rs, again)
            log = rs.geometry_log()
            assert log["pairs"] <= pairs and log["entries"] <= entries
            assert log["allocated"] == 0 and rs.bytes() == held, (log, rs.bytes(), held)
        now = rs.pointers()
        assert now[4:] == ptrs[4:] and now[:4] != ptrs[:4]
        watched = frame(rs)
        assert_planes(watched, planes, "watched frame after the update")
        for _ in range(3):
            rs.render()
        rs.sync()
        assert rs.finish() is False, "a planned frame after the update was incomplete and had to be redone"
        assert_planes(rs.readback(), watched, "planned frames after the update")
        ms = rs.geometry_times_ms()
        assert all(v > 0 for v in ms.values()), ms
    finally:
        rs.close()


def test_command_line_spin(tmp_path):
    """--spin through the command line's own loop (set_vertices with the index array at pose 1 only and turned normals at every pose,
    passes, denoise and AO on): every pose's files exist, and pose 2's image is, byte for byte, the one the same writer gives for a scene
    created fresh from the turned arrays at the camera --eye / --look-at / --fov set."""
    from opencl_render_amd import __main__ as cli, scene as S
    argv = ["--scene", "soup", "--triangles", "400", "--width", "96", "--height", "64", "--samples", "2", "--spin", "3", "--eye", "0.2", "0.1", "-0.5",
            "--fov", "40", "--out", str(tmp_path / "img.ppm"), "--passes", str(tmp_path / "p"), "--surface-passes", "--denoise", str(tmp_path / "d.pfm"),
            "--ao", str(tmp_path / "a.pfm"), "--ao-rays", "4"]
    assert cli.main(argv) == 0
    for i in range(3):
        for f in (f"img_{i:03d}.ppm", f"p_{i:03d}_alpha.pgm", f"p_{i:03d}_normal.pfm", f"d_{i:03d}.pfm", f"a_{i:03d}.pfm"):
            assert (tmp_path / f).stat().st_size > 0, f
    images = [(tmp_path / f"img_{i:03d}.ppm").read_bytes() for i in range(3)]
    assert len(set(images)) == 3  # the poses differ
    args = cli.parse_args(argv)
    sc = S.make_soup(96, 64, 400, 0.02, samples=2)
    eye, centre = np.float32([0.2, 0.1, -0.5]), np.float32([0, 0, 3])
    tl, lr, tb, inv = R.look_at_vectors(eye, centre, (0, 1, 0), np.radians(40.0), 96, 64)
    turned = GC.with_arrays(sc, R.spin_vertices(sc.vertex, centre, 2, 3), sc.tri_index, R.spin_directions(sc.tri_normal, 2, 3), lists=False)
    turned.eye = np.float32([0.2, 0.1, -0.5, 0.0])
    turned.eye_to_top_left, turned.left_to_right, turned.top_to_bottom, turned.pixel_size_inv = tl, lr, tb, inv
    turned.box_min, turned.grid_start, turned.grid_list = O.oracle_scene_grid(turned)
    turned.cam_start, turned.cam_end, turned.cam_list = O.oracle_camera_list(turned)
    rs = R.ResidentScene(turned, 0)
    try:
        planes = [p.reshape(64, 96) for p in frame(rs)]
    finally:
        rs.close()
    args.out = str(tmp_path / "fresh.ppm")
    args.passes = args.denoise = args.ao = None
    cli.write_view(args, dict(out=args.out, passes=None, denoise=None, ao=None), planes, None, None, None)
    assert (tmp_path / "fresh.ppm").read_bytes() == images[2]
