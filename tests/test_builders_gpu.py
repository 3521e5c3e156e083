"""GPU list builders (rt_build_device.hip) against the host builders (rt_builders.cpp) AND against the independent builder
oracle (oracle/rt_oracle_builders.c, a serial restatement of trianglelist.cpp that shares no code with either).  Camera
lists: the same triangles in the same pixels, every pixel's entries ascending, and the same storage sharing between equal
neighbouring lists (the reference's de-duplication, trianglelist.cpp:580-613) -- so Start, End and the list are compared as
arrays.  Parity of the builders against the reference itself stays unpinned (trianglelist.cpp cannot be compiled here)."""
import copy
import os

import numpy as np
import pytest

import builder_cases as BC
import oracle_lib as O
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu


def per_pixel_lists(sc):
    return [sc.cam_list[a:b] for a, b in zip(sc.cam_start.tolist(), sc.cam_end.tolist())]


def assert_same_lists(host, dev, label):
    assert len(host.cam_start) == len(dev.cam_start) == host.pixels
    n_host = host.cam_end.astype(np.int64) - host.cam_start.astype(np.int64)
    n_dev = dev.cam_end.astype(np.int64) - dev.cam_start.astype(np.int64)
    bad = np.nonzero(n_host != n_dev)[0]
    assert bad.size == 0, f"{label}: {bad.size} pixels differ in list length, first {bad[:5]} (host {n_host[bad[:5]]}, device {n_dev[bad[:5]]})"
    # flatten both in pixel order and compare at once
    order_h = np.concatenate([np.arange(a, b) for a, b in zip(host.cam_start.tolist(), host.cam_end.tolist())]) if n_host.sum() else np.zeros(0, np.int64)
    order_d = np.concatenate([np.arange(a, b) for a, b in zip(dev.cam_start.tolist(), dev.cam_end.tolist())]) if n_dev.sum() else np.zeros(0, np.int64)
    assert np.array_equal(host.cam_list[order_h], dev.cam_list[order_d]), f"{label}: list contents differ"


def with_big_triangles(sc, seed):
    """Adds triangles that cover large parts of the image (rectangles far above RT_BIG_RECT pixels), some partly off screen."""
    rng = np.random.default_rng(seed)
    extra = []
    for _ in range(6):
        z = rng.uniform(2.0, 4.0)
        centre = np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.2, 0.2) * z, z], np.float32)
        pts = centre + rng.uniform(-0.9, 0.9, (3, 3)).astype(np.float32) * np.float32(z * 0.5)
        pts[:, 2] = np.maximum(pts[:, 2], 1.5)
        extra.append(pts.astype(np.float32))
    extra = np.stack(extra)  # [k,3,3]
    k = len(extra)
    out = copy.copy(sc)
    v = np.zeros((3 * k, 4), np.float32)
    v[:, :3] = extra.reshape(-1, 3)
    base = sc.vertex.shape[0]
    out.vertex = np.concatenate([sc.vertex, v])
    idx = np.zeros((k, 4), np.int32)
    idx[:, 0] = base + 3 * np.arange(k); idx[:, 1] = idx[:, 0] + 1; idx[:, 2] = idx[:, 0] + 2
    out.tri_index = np.concatenate([sc.tri_index, idx])
    out.tri_material = np.concatenate([sc.tri_material, np.zeros(k, np.int32) + sc.tri_material[0]])
    out.tri_uv = np.concatenate([sc.tri_uv, np.zeros((3 * k, 2), np.float32)])
    n = np.zeros((3 * k, 4), np.float32); n[:, 2] = -1
    out.tri_normal = np.concatenate([sc.tri_normal, n])
    return out


@pytest.mark.parametrize("w,h,tris,edge,seed,big", [
    (300, 200, 6000, 0.15, 5, False),      # many candidates per pixel
    (640, 360, 60_000, 0.012, 77, False),  # small triangles
    (333, 177, 3000, 0.4, 9, True),        # odd size, triangles larger than the image, partly off screen
    (1920, 1080, 100_000, 0.01, 12345, True),
])
def test_device_camera_lists_equal_host_lists(w, h, tris, edge, seed, big):
    sc = S.make_soup(w, h, tris, edge, seed=seed, samples=1)
    if big:
        sc = with_big_triangles(sc, seed)
    host, dev = copy.copy(sc), copy.copy(sc)
    R.build_camera_list(host)
    ms = R.build_camera_list_device(dev, 0)
    assert ms > 0
    assert_same_lists(host, dev, f"{w}x{h}, {sc.triangle_count} triangles")
    # with the neighbour de-duplication on the device as well, the three arrays themselves are equal
    assert np.array_equal(host.cam_start, dev.cam_start), "Start (aliasing) differs"
    assert np.array_equal(host.cam_end, dev.cam_end), "End differs"
    assert np.array_equal(host.cam_list, dev.cam_list), "list storage differs"
    if sc.triangle_count <= 10_000:  # the serial oracle sorts 64-bit keys: keep it to the small cases
        import oracle_lib as O
        ostart, oend, olist = O.oracle_camera_list(sc)
        assert np.array_equal(dev.cam_start, ostart) and np.array_equal(dev.cam_end, oend) and np.array_equal(dev.cam_list, olist), \
            "device camera lists differ from the independent oracle"


@pytest.mark.parametrize("w,h,tris,edge,seed,big", [
    (300, 200, 6000, 0.15, 5, False),      # triangles over a few cells each: the one-thread fill, some spill to the workgroup fill
    (640, 360, 60_000, 0.012, 77, False),  # small triangles
    (333, 177, 3000, 0.4, 9, True),        # triangles over thousands of cells: the workgroup fill
    (1920, 1080, 100_000, 0.01, 12345, True),
])
def test_device_grid_equals_host_grid(w, h, tris, edge, seed, big):
    sc = S.make_soup(w, h, tris, edge, seed=seed, samples=1)
    if big:
        sc = with_big_triangles(sc, seed)
    host, dev = copy.copy(sc), copy.copy(sc)
    R.build_scene_grid(host)
    ms = R.build_scene_grid_device(dev, 0)
    assert ms > 0
    assert np.array_equal(host.box_min, dev.box_min), "split planes differ"
    assert len(host.grid_list) == len(dev.grid_list), f"pair count {len(host.grid_list)} vs {len(dev.grid_list)}"
    assert np.array_equal(host.grid_start, dev.grid_start), "cell starts differ"
    assert np.array_equal(host.grid_list, dev.grid_list), "cell lists differ"
    if sc.triangle_count <= 10_000:
        import oracle_lib as O
        obox, ostart, olist = O.oracle_scene_grid(sc)
        assert dev.box_min.tobytes() == obox.tobytes() and np.array_equal(dev.grid_start, ostart) and np.array_equal(dev.grid_list, olist), \
            "device grid differs from the independent oracle"


def test_frame_from_device_built_lists_matches_oracle():
    """The hot path on device-built lists: same planes as the CPU oracle on the host-built lists."""
    import os
    import oracle_lib as O
    sc = S.make_soup(320, 240, 20_000, 0.03, seed=21, samples=2)
    host = copy.copy(sc)
    R.build_lists(host)
    want = O.oracle_render(host, threads=os.cpu_count() or 1)
    dev = copy.copy(sc)
    R.build_camera_list_device(dev, 0)
    R.build_scene_grid_device(dev, 0)
    got = R.render_resident(dev, 0)
    for ch, g, w in zip("RGB", got, want):
        assert np.array_equal(g, w), f"plane {ch}: {(g != w).sum()} values differ"


# ---- every builder family (tests/builder_cases.py) against the independent oracle ----------------------------------------------


def assert_planes_equal(got, want, signed_zeros, label):
    """Byte for byte; in a scene with coordinates of both zero signs by value (-0 == +0): a plane taken at a run of zeros gets
    the sign of whichever zero each builder's sort put there (the device's radix sort puts every -0.0 first)."""
    if signed_zeros:
        assert np.array_equal(got, want), f"{label}: split planes differ in value"
        differ = got.view(np.uint32) != want.view(np.uint32)
        assert (got[differ] == 0).all(), f"{label}: split planes differ in more than the sign of a zero"
    else:
        assert got.tobytes() == want.tobytes(), f"{label}: split planes differ"


def device_lists(sc):
    dev = copy.copy(sc)
    R.build_camera_list_device(dev, 0)
    R.build_scene_grid_device(dev, 0)
    return dev, R.build_log()


def assert_device_equals_oracle(dev, ocam, ogrid, label, signed_zeros=False):
    ostart, oend, olist = ocam
    assert np.array_equal(dev.cam_start, ostart), f"{label}: camera Start differs from the oracle"
    assert np.array_equal(dev.cam_end, oend), f"{label}: camera End differs from the oracle"
    assert np.array_equal(dev.cam_list, olist), f"{label}: camera list differs from the oracle"
    obox, ogstart, oglist = ogrid
    assert_planes_equal(dev.box_min, obox, signed_zeros, label)
    assert np.array_equal(dev.grid_start, ogstart), f"{label}: grid Start differs from the oracle"
    assert np.array_equal(dev.grid_list, oglist), f"{label}: grid list differs from the oracle"


@pytest.mark.parametrize("name", BC.NAMES)
def test_device_builders_equal_oracle_on_every_family(name):
    sc = BC.make(name)
    R.tune("reset", 0)
    dev, log = device_lists(sc)
    assert_device_equals_oracle(dev, O.oracle_camera_list(sc), O.oracle_scene_grid(sc), name, sc.meta.get("signed_zeros", False))
    T = sc.triangle_count
    # the build log adds up, and a default build fills once
    assert log["cam_thread"] + log["cam_group"] == T and log["grid_thread"] + log["grid_group"] == T, log
    assert log["cam_entries"] == int((dev.cam_end.astype(np.int64) - dev.cam_start).sum()), log
    assert log["pairs"] == len(dev.grid_list) and log["attempts"] == 1 and log["key_cap_first"] == max(32 * T, 1 << 22), log
    assert log["grid_batches"] == -(-log["grid_group"] // 64), log
    if name == "boundary":  # every 1 024-pixel rectangle by one thread, every 1 025-pixel one by a workgroup
        areas = sc.meta["rect_area"]
        assert log["cam_thread"] == areas.count(BC.BIG_RECT) and log["cam_group"] == areas.count(BC.BIG_RECT + 1), log
    if name in ("room", "obj"):  # every triangle over more than 48 cells: the key buffer grows for their overlap boxes
        assert log["grid_group"] == T and log["grew"] == 1 and log["key_cap_final"] >= log["pairs"] > log["key_cap_first"], log
    if name == "room":  # 146 big triangles: three batches through the same 64 bitmaps and passmaps
        assert log["grid_batches"] >= 2, log


@pytest.mark.parametrize("name", ["signed_zeros", "room"])
def test_frame_from_device_lists_equals_oracle_frame_from_host_lists(name):
    """Whatever zero sign the device's planes carry, the frame must be the oracle's on the host builder's lists."""
    sc = BC.make(name)
    host = R.build_lists(copy.copy(sc))
    want = O.oracle_render(host, threads=os.cpu_count() or 1)
    dev, _ = device_lists(sc)
    got = R.render_resident(dev, 0)
    for ch, g, w in zip("RGB", got, want):
        assert np.array_equal(g, w), f"{name}, plane {ch}: {(g != w).sum()} values differ"


def small_and_total_pairs(sc):
    """(pairs of the triangles a thread fills on its own, all pairs), from the host grid: a triangle over at most 48 cells
    (RT_FILL_LOCAL) is filled by one thread."""
    host = R.build_lists(copy.copy(sc))
    per_tri = np.bincount(host.grid_list, minlength=sc.triangle_count)
    return int(per_tri[per_tri <= 48].sum()), len(host.grid_list)


@pytest.mark.parametrize("where", ["below_small_pairs", "between_small_and_all_pairs"])
def test_grid_key_buffer_overflow_paths(where):
    """build_key_cap below the one-thread fills' pairs: the first fill overflows and the grid is filled a second time into a buffer
    of the counted size.  Between those pairs and all pairs: the buffer grows for the big triangles before they are filled."""
    sc = BC.make("soup_72x56")
    small, total = small_and_total_pairs(sc)
    assert 1000 < small < total - 1000
    cap = small // 2 if where == "below_small_pairs" else (small + total) // 2
    try:
        R.tune("build_key_cap", cap)
        dev, log = device_lists(sc)
    finally:
        R.tune("reset", 0)
    assert_device_equals_oracle(dev, O.oracle_camera_list(sc), O.oracle_scene_grid(sc), f"key capacity {cap}")
    assert log["key_cap_first"] == cap and log["pairs"] == total and log["key_cap_final"] >= total, log
    if where == "below_small_pairs":
        assert log["attempts"] == 2, log
    else:
        assert log["attempts"] == 1 and log["grew"] == 1, log


def test_device_builders_refuse_lists_above_the_limit():
    """build_list_limit stands in for 2^32 - 1: one entry more than the limit is refused with -3 (the camera builder before it
    allocates or fills the list), exactly the limit is built."""
    sc = BC.make("soup_200x150")
    host = R.build_lists(copy.copy(sc))
    entries, pairs = int((host.cam_end.astype(np.int64) - host.cam_start).sum()), len(host.grid_list)
    try:
        R.tune("build_list_limit", entries - 1)
        with pytest.raises(RuntimeError, match=r"rtHipBuildCameraListDevice failed \(-3\)"):
            R.build_camera_list_device(copy.copy(sc), 0)
        assert R.build_log()["cam_entries"] == entries
        R.tune("build_list_limit", pairs - 1)
        with pytest.raises(RuntimeError, match=r"rtHipBuildSceneGridDevice failed \(-3\)"):
            R.build_scene_grid_device(copy.copy(sc), 0)
        assert R.build_log()["pairs"] == pairs
        R.tune("build_list_limit", max(entries, pairs))
        dev, _ = device_lists(sc)
    finally:
        R.tune("reset", 0)
    for k in ("cam_start", "cam_end", "cam_list", "box_min", "grid_start", "grid_list"):
        assert np.array_equal(getattr(dev, k), getattr(host, k)), k
