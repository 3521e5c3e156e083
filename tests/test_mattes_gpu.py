"""Mattes on the MI355X (run with -m gpu): rtHipSceneMattes / rtHipSceneMattesDevice give, bit for bit, what the definition of
include/raytrace_hip.h gives when matte_oracle.py restates it with the oracle's generator and triangle test -- for every kind, overflowing
and exact layer tables, chunked launches, sample windows, tile deals, device and host arrays, after scene moves and edits -- and a call
leaves frames, passes and the scene's byte count alone.  The per-sample ids of each scene are computed once (module scope)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import matte_oracle as MO
import scenarios as SC
from conftest import load_golden_scene
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu
NONE = MO.NONE
F32 = np.float32
KEYS = ("select", "layer_id", "layer_coverage", "rest")
COMBOS = [(0, 1), (0, 2), (0, 8), (16, 0), (3, 4)]  # (M, K)


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the matte tests cannot run (and the product has no CPU fallback)")


@pytest.fixture(autouse=True)
def fresh_tuning():
    R.tune("reset", 0)
    yield
    R.tune("reset", 0)


# name -> (scene, N, f, C, most distinct triangles the issue's census found in a pixel)
def _soup(name):
    if name == "A":
        return S.make_soup(40, 32, 500, 0.3, seed=7, name="matte_A"), 8, 0, 8, 5
    if name == "B":
        return S.make_soup(40, 32, 4000, 0.06, seed=8, name="matte_B"), 16, 0, 16, 5
    if name == "C":  # 2 x 2 tiles, ragged on both edges; S = C = 3 for the cross-check against the frame's passes
        return S.make_soup(160, 136, 2500, 0.08, seed=9, samples=3, name="matte_C"), 3, 0, 3, 3
    raise KeyError(name)


_scenes, _ids = {}, {}


def scene(name):
    if name not in _scenes:
        if name in "ABC":
            sc, N, f, C_, D = _soup(name)
            R.build_lists(sc)
        elif name == "room":
            sc = SC._axis_scene("matte_room", [SC._sun(4, (0.0, -1.0, 0.0), 0.8)])
            N, f, C_, D = 2, 0, 2, 2
        else:
            sc = load_golden_scene(name)[0]
            N, f, C_, D = sc.sample_count, 0, sc.sample_count, 2
        _scenes[name] = (sc, N, f, C_, D)
    return _scenes[name]


def ids_of(name, window=None):
    """The oracle's per-sample triangles of a scene under its own window or `window` = (N, f, C): computed once, never changed."""
    sc, N, f, C_, _ = scene(name)
    key = (name,) + tuple(window or (N, f, C_))
    if key not in _ids:
        _ids[key] = MO.sample_ids(sc, *key[1:])
        _ids[key].setflags(write=False)
    return _ids[key]


def want(name, table, select, K, window=None):
    sc, N, f, C_, _ = scene(name)
    C_ = window[2] if window else C_
    return MO.mattes(ids_of(name, window), table, select, K, C_, shape=(sc.height, sc.width))


def assert_same(got, want_, what):
    for k in KEYS:
        if k not in got:
            assert want_[k].shape[0] == 0, f"{what}: {k} missing"
            continue
        g, w = np.asarray(got[k]), want_[k]
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k} is {g.dtype} {g.shape}, expected {w.dtype} {w.shape}"
        bad = np.flatnonzero(g.view(np.uint32).reshape(-1) != w.view(np.uint32).reshape(-1))
        assert bad.size == 0, (f"{what}: {k} differs in {bad.size}/{w.size} values, first at {bad[0]}: "
                               f"{g.reshape(-1)[bad[:4]]} vs {w.reshape(-1)[bad[:4]]}")


def selection(ids, M, T):
    """M ids to select: the most frequent ones, then an id nothing hits, then the most frequent again (a repeated id)."""
    hit = ids[ids != NONE]
    values, counts = np.unique(hit, return_counts=True)
    ranked = [int(v) for v in values[np.argsort(-counts, kind="stable")]]
    unhit = next(t for t in range(T) if t not in set(ranked))
    return (ranked[:max(M - 2, 1)] + [unhit, ranked[0]])[:M] if M else []


def window_kw(name, window=None):
    _, N, f, C_, _ = scene(name)
    N, f, C_ = window or (N, f, C_)
    return dict(total=N, first=f, samples=C_)


def test_the_scenes_overflow_small_tables_and_fit_large_ones():
    """What the comparisons below rely on, asserted from the oracle so that a scene change cannot make them vacuous."""
    assert MO.distinct_histogram(ids_of("A")) == [326, 560, 299, 83, 10, 2]
    assert MO.distinct_histogram(ids_of("B")) == [239, 396, 345, 203, 76, 16, 3, 2]
    assert MO.distinct_histogram(ids_of("C")) == [15749, 5459, 546, 6]
    for name in "ABC":
        D = scene(name)[4]
        for K in (1, 2, 4, 8):
            w = want(name, None, [], K)
            used = (w["layer_count"] > 0).sum(0)
            for n in range(1, min(K, D) + 1):
                assert (used == n).any(), f"{name}: no pixel with {n} used slots at K = {K}"
            total = w["layer_count"].sum(0).astype(np.int64) + w["rest_count"] + w["none_count"]
            assert (total == scene(name)[3]).all()
        if name in "AB":
            assert (want(name, None, [], 2)["rest_count"] > 0).sum() >= 50
        assert (want(name, None, [], 2)["rest_count"] > 0).any()
        assert not want(name, None, [], 8)["rest_count"].any()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_triangle_kind_matches_the_oracle(name):
    sc = scene(name)[0]
    rs = R.ResidentScene(sc)
    try:
        for M, K in COMBOS:
            sel = selection(ids_of(name), M, sc.triangle_count)
            assert len(sel) == M and (M < 3 or (sel[-1] == sel[0] and not (ids_of(name) == sel[-2]).any()))
            got = rs.mattes(kind="triangle", select=sel, layers=K, **window_kw(name))
            w = want(name, None, sel, K)
            assert_same(got, w, f"{name} M={M} K={K}")
            if M:
                assert (w["select"][0] > 0).any() and not w["select"][-2].any() and np.array_equal(w["select"][0], w["select"][-1])
        ms = rs.matte_times_ms()
        assert ms["count"] > 0 and ms["finish"] > 0
    finally:
        rs.close()


@pytest.mark.parametrize("name", ["mixed_materials_textured", "no_material"])
def test_material_kind_on_the_goldens(name):
    sc = scene(name)[0]
    mats = np.asarray(sc.tri_material, np.int32)
    ids = ids_of(name)
    hit = ids[ids != NONE]
    assert (mats[hit] < 0).any() and (mats[hit] >= 0).any()  # samples on triangles without a material, and on ones with
    table = MO.material_table(mats)
    sel = sorted(set(int(m) for m in mats if m >= 0))[:5] + [int(mats.max()) + 7]  # every id in use (five at most), and one that is not
    rs = R.ResidentScene(sc)
    try:
        for K in (1, 8):
            got = rs.mattes(kind="material", select=sel, layers=K)  # the defaults: the scene's own samples
            w = want(name, table, sel, K)
            assert_same(got, w, f"{name} K={K}")
        only_none = (MO.table_ids(ids, table) == NONE).all(1) & (ids != NONE).any(1)  # hit pixels all of whose hits are id -1
        assert only_none.any()
        assert not got["layer_coverage"].reshape(8, -1)[:, only_none].any() and (got["layer_id"].reshape(8, -1)[:, only_none] == NONE).all()
        assert not got["select"].reshape(len(sel), -1)[:, only_none].any() and not got["rest"].reshape(-1)[only_none].any()
    finally:
        rs.close()


def group_table(T, seed=5):
    """Many triangles in few groups, some in none, some group ids above T."""
    rng = np.random.default_rng(seed)
    table = rng.integers(0, 5, T).astype(np.uint32)
    table[rng.random(T) < 0.15] = NONE
    big = rng.random(T) < 0.2
    table[big] = rng.choice(np.array([T + 1, 1_000_000, 0xFFFFFFFE], np.uint32), int(big.sum()))
    return table


def test_group_kind_with_a_seeded_table():
    sc = scene("A")[0]
    table = group_table(sc.triangle_count)
    hit = ids_of("A")[ids_of("A") != NONE]
    seen = set(int(v) for v in table[hit])
    assert NONE in seen and {1_000_000, 0xFFFFFFFE} & seen and len(seen) <= 9
    sel = [0, 3, 0xFFFFFFFE, sc.triangle_count + 1, 77, 3]
    rs = R.ResidentScene(sc)
    try:
        with pytest.raises(RuntimeError, match="group table"):
            rs.mattes(kind="group", **window_kw("A"))
        rs.set_matte_groups(table)
        for K in (2, 8):
            assert_same(rs.mattes(kind="group", select=sel, layers=K, **window_kw("A")), want("A", table, sel, K), f"groups from the host, K={K}")
        assert (want("A", table, sel, 2)["rest_count"] > 0).any() and not want("A", table, sel, 8)["rest_count"].any()
        other = np.roll(table, 1)
        rs.set_matte_groups(torch.as_tensor(other.view(np.int32), device="cuda:0"))  # from device memory, replacing the table in place
        assert_same(rs.mattes(kind="group", select=sel, layers=8, **window_kw("A")), want("A", other, sel, 8), "groups from the device")
        host = np.zeros(4, np.uint32)
        assert R.lib().rtHipSceneSetMatteGroups(rs.handle, host.ctypes.data_as(C.c_void_p), 1) == -1  # a host pointer called a device one
        assert "not device memory" in R.last_error()
        assert_same(rs.mattes(kind="group", select=sel, layers=8, **window_kw("A")), want("A", other, sel, 8), "the table a refusal left")
    finally:
        rs.close()


def test_mesh_kind_on_a_room_through_python():
    sc = scene("room")[0]
    table = np.asarray(sc.tri_mesh, np.int32).view(np.uint32)
    meshes = sorted(set(int(v) for v in table))
    assert len(meshes) >= 5
    w = want("room", table, meshes[:16], 4)
    assert ((w["layer_count"] > 0).sum(0) == 2).sum() >= 50  # edge pixels between two meshes
    rs = R.ResidentScene(sc)
    try:
        before = rs.bytes()
        assert_same(rs.mattes(kind="mesh", select=meshes[:16], layers=4), w, "room, mesh groups")
        grown = rs.bytes()
        assert grown > before
        assert_same(rs.mattes(kind="mesh", select=meshes[:16], layers=4), w, "room, mesh groups again")
        assert rs.bytes() == grown  # the table is installed once
        soup = R.ResidentScene(scene("A")[0])
        try:
            with pytest.raises(ValueError, match="tri_mesh"):
                soup.mattes(kind="mesh")
        finally:
            soup.close()
    finally:
        rs.close()


def test_chunked_launches_give_identical_outputs():
    sc = scene("B")[0]
    sel = selection(ids_of("B"), 3, sc.triangle_count)
    w = want("B", None, sel, 4)
    rs = R.ResidentScene(sc)
    try:
        for chunk in (1, 3, 64):  # 16 samples: 16 launches, 5 full ones and one of 1, one launch
            R.tune("matte_chunk", chunk)
            assert_same(rs.mattes(select=sel, layers=4, **window_kw("B")), w, f"matte_chunk {chunk}")
            assert_same(rs.mattes(select=sel, layers=2, **window_kw("B")), want("B", None, sel, 2), f"matte_chunk {chunk}, K=2")
    finally:
        rs.close()


def test_sample_windows():
    sc = scene("A")[0]
    window = (16, 4, 8)
    assert not np.array_equal(ids_of("A"), ids_of("A", window))
    rs = R.ResidentScene(sc)
    try:
        S_ = sc.sample_count
        assert rs.matte_defaults() == dict(kind="triangle", select=(), layers=4, total=S_, first=0, samples=S_)
        assert_same(rs.mattes(select=[3], layers=8, **window_kw("A", window)), want("A", None, [3], 8, window), "window {16, 4, 8}")
        rs.set_sample_window(16, 4)
        assert rs.matte_defaults()["total"] == S_  # set, not yet used by a frame
        rs.render()
        rs.readback()
        assert rs.matte_defaults() == dict(kind="triangle", select=(), layers=4, total=16, first=4, samples=S_)
        assert rs.sample_window()["last"]["total"] == 16 and rs.sample_window()["next"]["first"] == 4  # the call left the window alone
        got = rs.mattes(layers=2)  # the defaults: sample id 5 of 16
        assert_same(got, MO.mattes(ids_of("A", window)[:, :S_], None, [], 2, S_, shape=(sc.height, sc.width)), "the last frame's window")
    finally:
        rs.close()


def test_layers_agree_with_the_alpha_and_triangle_passes():
    """Independent of the new oracle: on C with C = S, f = 0 and K = 8 the layer counts add up to the ALPHA pass's hits, and layer 0 is
    the TRIANGLE pass's id wherever the pixel's samples all hit one triangle."""
    sc = scene("C")[0]
    S_ = sc.sample_count
    assert S_ == 3
    rs = R.ResidentScene(sc)
    try:
        rs.set_passes(alpha=True, triangle=True)
        rs.render()
        passes = rs.readback_passes()
        got = rs.mattes(layers=8)
    finally:
        rs.close()
    counts = np.rint(got["layer_coverage"].astype(np.float64) * S_).astype(np.int64)
    assert np.array_equal((counts.astype(F32) / F32(S_)).view(np.uint32), got["layer_coverage"].view(np.uint32))
    hits = counts.sum(0)
    assert not got["rest"].any() and hits.max() == S_ and (hits == 0).any()
    assert np.array_equal(passes["alpha"], (hits * 65535 // S_).astype(np.uint16))
    one = (counts[0] == S_)
    assert one.sum() > 1000 and np.array_equal(got["layer_id"][0][one], passes["triangle"][one])
    seen = passes["triangle"] != NONE  # sample 1's triangle is one of the pixel's layers
    assert seen.any() and (got["layer_id"] == passes["triangle"][None])[:, seen].any(0).all()


def test_disjoint_tile_deals_compose_one_image():
    sc = scene("C")[0]
    sel = selection(ids_of("C"), 3, sc.triangle_count)
    w = want("C", None, sel, 4)
    H, W = sc.height, sc.width
    host = dict(select=np.full((3, H, W), -7.0, F32), layer_id=np.full((4, H, W), 12345, np.uint32),
                layer_coverage=np.full((4, H, W), -7.0, F32), rest=np.full((H, W), -7.0, F32))
    dev = {k: torch.as_tensor(v.view(np.int32) if k == "layer_id" else v, device="cuda:0").clone() for k, v in host.items()}
    parts = []
    try:
        for rank in range(2):
            tiles = R.tiles_of_rank(W, H, rank, 2)
            parts.append(R.ResidentScene(sc, 0, tiles, like=parts[0] if parts else None))
            assert parts[-1].mattes(select=sel, layers=4, out=host) is host
            parts[-1].mattes(select=sel, layers=4, out=dev)
            torch.cuda.synchronize()
            if rank == 0:  # pixels of foreign tiles keep the sentinel
                mine = np.zeros((H, W), bool)
                for t in tiles:
                    ty, tx = divmod(int(t), (W + R.TILE - 1) // R.TILE)
                    mine[ty * R.TILE:(ty + 1) * R.TILE, tx * R.TILE:(tx + 1) * R.TILE] = True
                assert mine.any() and not mine.all()
                for arrays in (host, {k: v.cpu().numpy().view(host[k].dtype) for k, v in dev.items()}):
                    assert (arrays["rest"][~mine] == -7.0).all() and (arrays["select"][:, ~mine] == -7.0).all()
                    assert (arrays["layer_id"][:, ~mine] == 12345).all() and (arrays["layer_coverage"][:, ~mine] == -7.0).all()
                    assert np.array_equal(arrays["rest"][mine], w["rest"][mine])
    finally:
        for p in parts:
            p.close()
    assert_same(host, w, "two instances composed (host)")
    assert_same({k: v.cpu().numpy().view(host[k].dtype) for k, v in dev.items()}, w, "two instances composed (device)")


def test_host_and_device_entries_agree_on_shuffled_partial_tiles():
    """Slot order that is not image order, one slot mostly outside the image: the host entry point's arrays are the device entry
    point's, bit for bit, other tiles' pixels left alone by both."""
    sc, tiles = SC.shuffled_tiles(), SC.SHUFFLED_TILES
    H, W = sc.height, sc.width
    host = dict(select=np.full((2, H, W), -7.0, F32), layer_id=np.full((3, H, W), 12345, np.uint32),
                layer_coverage=np.full((3, H, W), -7.0, F32), rest=np.full((H, W), -7.0, F32))
    dev = {k: torch.as_tensor(v.view(np.int32) if k == "layer_id" else v, device="cuda:0").clone() for k, v in host.items()}
    rs = R.ResidentScene(sc, 0, tiles)
    try:
        rs.mattes(select=(5, 17), layers=3, out=host)
        rs.mattes(select=(5, 17), layers=3, out=dev)
        torch.cuda.synchronize()
    finally:
        rs.close()
    mine = SC.tiles_mask(sc, tiles)
    assert_same(host, {k: v.cpu().numpy().view(host[k].dtype) for k, v in dev.items()}, "tiles 3, 0")
    assert (host["rest"][~mine] == -7.0).all() and (host["layer_id"][:, ~mine] == 12345).all() and (host["rest"][mine] >= 0).all()
    assert (host["layer_coverage"][0][128:, 128:] > 0).any() and (host["layer_coverage"][0][:128, :128] > 0).any()


def test_device_arrays_equal_host_arrays():
    sc = scene("B")[0]
    sel = selection(ids_of("B"), 3, sc.triangle_count)
    w = want("B", None, sel, 4)
    H, W = sc.height, sc.width
    dev = torch.device("cuda", 0)
    rs = R.ResidentScene(sc)
    try:
        def tensors():
            return dict(select=torch.full((3, H, W), -1.0, device=dev), layer_id=torch.full((4, H, W), 99, dtype=torch.int32, device=dev),
                        layer_coverage=torch.full((4, H, W), -1.0, device=dev), rest=torch.full((H, W), -1.0, device=dev))

        def as_numpy(t):
            return {k: v.cpu().numpy().view(np.uint32 if k == "layer_id" else F32) for k, v in t.items()}

        host = rs.mattes(select=sel, layers=4, **window_kw("B"))
        assert_same(host, w, "host arrays")
        out = tensors()
        assert rs.mattes(select=sel, layers=4, out=out, **window_kw("B")) is out
        torch.cuda.synchronize()
        assert_same(as_numpy(out), w, "device arrays (torch, current stream)")
        side = torch.cuda.Stream(dev)  # a foreign stream, and twice on it with another table shape between: the state is reused in order
        out2, out3 = tensors(), tensors()
        before = rs.bytes()
        with torch.cuda.stream(side):
            rs.mattes(select=sel, layers=4, out=out2, **window_kw("B"))
            rs.mattes(select=sel, layers=2, out={k: v[:2] if k.startswith("layer") else v for k, v in out3.items()}, **window_kw("B"))
            rs.mattes(select=sel, layers=4, out=out2, **window_kw("B"))
        torch.cuda.synchronize()
        assert rs.bytes() == before  # the scratch already fitted: no allocation
        assert_same(as_numpy(out2), w, "device arrays (foreign stream)")
        w2 = want("B", None, sel, 2)
        assert_same({k: v[:2] if k.startswith("layer") else v for k, v in as_numpy(out3).items()}, w2, "K = 2 between")
        only = dict(rest=torch.full((H, W), -1.0, device=dev))  # a subset of the outputs
        rs.mattes(select=sel, layers=4, out=only, **window_kw("B"))
        torch.cuda.synchronize()
        assert np.array_equal(only["rest"].cpu().numpy(), w["rest"])
        with pytest.raises(ValueError):
            rs.mattes(layers=4, out=dict(rest=torch.zeros((H, W + 1), device=dev)))
        with pytest.raises(ValueError):
            rs.mattes(layers=4, out=dict(rest=np.zeros((H, W), np.float64)))
    finally:
        rs.close()


def fresh_mattes(sc, groups=None, **kw):
    rs = R.ResidentScene(sc)
    try:
        if groups is not None:
            rs.set_matte_groups(groups)
        return rs.mattes(**kw)
    finally:
        rs.close()


def test_mattes_follow_the_scene():
    sc = scene("A")[0]
    kw = dict(select=[3, 11], layers=8, **window_kw("A"))
    table = group_table(sc.triangle_count, seed=6)
    moved = copy.copy(sc)
    moved.eye = np.asarray(sc.eye, F32).copy()
    moved.eye[:3] += F32([0.05, -0.03, 0.02])
    R.build_lists(moved)
    bent = copy.copy(moved)
    bent.vertex = np.asarray(moved.vertex, F32).copy()
    bent.vertex[:, 0] += F32(0.1) * np.sin(np.arange(len(bent.vertex), dtype=F32))
    R.build_lists(bent)
    rs = R.ResidentScene(sc)
    try:
        home = rs.mattes(**kw)
        assert_same(home, want("A", None, [3, 11], 8), "before any move")
        rs.set_camera(moved.eye, moved.eye_to_top_left, moved.left_to_right, moved.top_to_bottom, moved.pixel_size_inv)
        after_camera = rs.mattes(**kw)
        assert_same(after_camera, fresh_mattes(moved, **kw), "after set_camera")
        assert not np.array_equal(after_camera["layer_id"], home["layer_id"])
        rs.set_matte_groups(table)  # installed before the geometry update, in effect after it
        rs.set_vertices(bent.vertex, bent.tri_index)  # (a scene drops the index array it was created with: the first update brings one)
        after_vertices = rs.mattes(**kw)
        assert_same(after_vertices, fresh_mattes(bent, **kw), "after set_vertices")
        assert not np.array_equal(after_vertices["layer_coverage"], after_camera["layer_coverage"])
        gkw = dict(kw, kind="group", select=[0, 3])
        assert_same(rs.mattes(**gkw), fresh_mattes(bent, groups=table, **gkw), "the group table after a geometry update")
    finally:
        rs.close()
    gold = scene("mixed_materials_textured")[0]
    mats = np.asarray(gold.tri_material, np.int32)
    count = int(mats.max()) + 1
    edited = copy.copy(gold)
    edited.tri_material = np.where(mats >= 0, (mats + 1) % count, mats).astype(np.int32)
    edited.tri_material[::7] = -1
    mkw = dict(kind="material", select=list(range(count)), layers=8)
    rs = R.ResidentScene(gold)
    try:
        first = rs.mattes(**mkw)
        rs.set_materials(tri_material=edited.tri_material)
        after_edit = rs.mattes(**mkw)
        assert_same(after_edit, fresh_mattes(edited, **mkw), "after set_materials(tri_material=...)")
        assert_same(after_edit, want("mixed_materials_textured", MO.material_table(edited.tri_material), mkw["select"], 8), "... and the oracle")
        assert not np.array_equal(after_edit["select"], first["select"])
    finally:
        rs.close()


def test_a_call_leaves_the_rest_alone():
    sc = load_golden_scene("lambert_distant")[0]
    T = sc.triangle_count
    quiet, rs = R.ResidentScene(sc), R.ResidentScene(sc)
    try:
        for r in (quiet, rs):
            r.set_passes(alpha=True, depth=True, triangle=True, normal=True, albedo=True)
            r.render()
        planes = [p.copy() for p in rs.readback()]
        passes = rs.readback_passes()
        quiet.readback()
        assert quiet.bytes() == rs.bytes()  # (the scene that never calls: what every scene cost before there were mattes)
        before = rs.bytes()
        window = rs.sample_window()
        rs.mattes(select=[1, 2], layers=4)
        state = rs.bytes()
        tiles = len(rs.tiles)
        assert state - before >= tiles * (2 + 2 * 4 + 1) * R.TILE * R.TILE * 4
        for _ in range(2):
            rs.mattes(select=[5, 6], layers=4)
            rs.mattes(select=[5], layers=2)  # fewer words per pixel: fits
            assert rs.bytes() == state
        rs.mattes(select=[1, 2, 3], layers=8)
        assert rs.bytes() > state  # more words per pixel: grown
        state = rs.bytes()
        rs.set_matte_groups(np.zeros(T, np.uint32))
        assert rs.bytes() - state >= 4 * T
        rs.mattes(kind="group", layers=1)
        rs.set_matte_groups(None)
        assert rs.bytes() == state  # the table's bytes are given back
        assert quiet.bytes() == before
        assert rs.sample_window() == window
        assert all(np.array_equal(a, b) for a, b in zip(planes, rs.readback()))  # the tile buffer is untouched
        rs.render()
        assert all(np.array_equal(a, b) for a, b in zip(planes, rs.readback()))
        again = rs.readback_passes()
        for k in passes:
            assert np.array_equal(np.asarray(passes[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8)), k
    finally:
        quiet.close()
        rs.close()
    mega = R.ResidentScene(scene("A")[0])  # the pass does not depend on the pipeline
    try:
        mega.set_pipeline(R.PIPELINE_MEGAKERNEL)
        assert_same(mega.mattes(select=[3], layers=8, **window_kw("A")), want("A", None, [3], 8), "megakernel pipeline")
    finally:
        mega.close()


def test_refusals_launch_nothing():
    sc = scene("A")[0]
    H, W = sc.height, sc.width
    L = R.lib()
    dev = torch.device("cuda", 0)
    rs = R.ResidentScene(sc)
    try:
        sel = torch.full((2, H, W), -3.0, device=dev)
        lid = torch.full((4, H, W), 77, dtype=torch.int32, device=dev)
        cov = torch.full((4, H, W), -3.0, device=dev)
        rest = torch.full((H, W), -3.0, device=dev)
        d = [C.c_void_p(t.data_ptr()) for t in (sel, lid, cov, rest)]
        hsel, hlid, hcov, hrest = (np.full((2, H, W), -3.0, F32), np.full((4, H, W), 77, np.uint32), np.full((4, H, W), -3.0, F32),
                                   np.full((H, W), -3.0, F32))
        h = [a.ctypes.data_as(C.c_void_p) for a in (hsel, hlid, hcov, hrest)]

        def params(**kw):
            p = R.MatteParams(kind=0, total=8, first=0, samples=8, selectCount=2, layers=4)
            p.select[0], p.select[1] = 1, 2
            for k, v in kw.items():
                setattr(p, k, v)
            return p

        def refused(p, dptrs=d, hptrs=h, text=None):
            for rc in (L.rtHipSceneMattesDevice(rs.handle, p, *dptrs, None), L.rtHipSceneMattes(rs.handle, p, *hptrs)):
                assert rc == -1
                assert R.last_error() and (text is None or text in R.last_error()), R.last_error()

        before = rs.bytes()
        good = params()
        refused(C.byref(params(kind=2)), text="group table")                                    # kind GROUP without a table
        refused(C.byref(good), dptrs=[None] * 4, hptrs=[None] * 4, text="every output is null")  # all outputs NULL
        for bad in (params(kind=3), params(total=0), params(samples=0), params(samples=65537, total=1 << 20), params(first=1),
                    params(selectCount=17), params(layers=9), params(selectCount=0, layers=0)):   # a failed check
            refused(C.byref(bad))
        none = params()
        none.select[1] = NONE
        refused(C.byref(none), text="select[1]")
        refused(C.byref(params(selectCount=0)), text="selectCount 0")                           # select given with M = 0
        refused(C.byref(params(layers=0)), text="layers 0")                                      # a layer output given with K = 0
        refused(None)
        assert L.rtHipSceneMattesDevice(None, C.byref(good), *d, None) == -1
        assert L.rtHipSceneMattes(None, C.byref(good), *h) == -1
        for i in range(4):                                                                       # a host pointer to the device call
            mixed = list(d)
            mixed[i] = h[i]
            assert L.rtHipSceneMattesDevice(rs.handle, C.byref(good), *mixed, None) == -1
            assert "not device memory" in R.last_error()
        torch.cuda.synchronize()
        assert rs.bytes() == before  # not even the scratch was made
        assert (sel == -3.0).all() and (lid == 77).all() and (cov == -3.0).all() and (rest == -3.0).all()
        assert (hsel == -3.0).all() and (hlid == 77).all() and (hcov == -3.0).all() and (hrest == -3.0).all()
        assert rs.matte_times_ms() == dict(count=0.0, finish=0.0)
        with pytest.raises(ValueError):
            rs.mattes(layers=9)
        with pytest.raises(ValueError):
            rs.mattes(select=[NONE])
        assert L.rtHipSceneMattesDevice(rs.handle, C.byref(good), *d, None) == 0                # and the good call goes through
        torch.cuda.synchronize()
        assert_same(dict(select=sel.cpu().numpy(), layer_id=lid.cpu().numpy().view(np.uint32), layer_coverage=cov.cpu().numpy(),
                         rest=rest.cpu().numpy()), want("A", None, [1, 2], 4), "after the refusals")
    finally:
        rs.close()


def test_command_line_writes_mattes_and_layers(tmp_path):
    from opencl_render_amd import __main__ as M
    args = ["--scene", "soup", "--width", "64", "--height", "48", "--samples", "4", "--triangles", "20000", "--out", str(tmp_path / "img.bmp"),
            "--mattes", str(tmp_path / "m"), "--matte-kind", "triangle", "--matte-layers", "3"]
    sc = S.make_soup(64, 48, 20000, 0.02, samples=4)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    first = fresh_mattes(sc, layers=3)
    top = [int(v) for v in np.unique(first["layer_id"][0][first["layer_id"][0] != NONE])[:2]]
    assert len(top) == 2
    assert M.main(args + ["--matte-select", ",".join(str(v) for v in top)]) == 0
    w = fresh_mattes(sc, select=top, layers=3)
    layers = np.load(tmp_path / "m_layers.npz")
    for k in ("layer_id", "layer_coverage", "rest"):
        assert np.array_equal(layers[k], w[k]), k
    for m, i in enumerate(top):
        with open(tmp_path / f"m_matte_{i}.pgm", "rb") as f:
            assert f.readline().strip() == b"P5"
            assert [int(v) for v in f.readline().split()] == [64, 48]
            assert int(f.readline()) == 255
            got = np.frombuffer(f.read(), np.uint8).reshape(48, 64)
        u16 = (w["select"][m] * F32(65535.0)).astype(np.uint16)
        assert u16.any() and np.array_equal(got, (u16 >> 8).astype(np.uint8))
