"""The scene upload's device side on the MI355X (run with -m gpu): the arrays a resident scene holds -- read back through
rtHipTestSceneView -- against prep_oracle.py, bit for bit, and the refusals of a bad scene with the legal neighbour of each.

Dense grid view (block words, the whole 50 MB sparse block table, pair records), triangle records, tile-major camera ranges, cellLut and
planesTame: every element is compared, on every golden scene, on synthetic grids that hold the layout's edges by construction
(prep_cases.synthetic_grids) and on a 1M-triangle soup.  The one sample in this file is the soup's consumer-side decode: decode_cell runs
on a fixed sample of 100 000 of its non-empty cells (every non-empty cell everywhere else).

Refusals: every family starts with the nearest offending value (== count, list size + 1) and goes on to the far ones (-1, INT_MIN) in the
same function, so that a missing check ends the function at the value that would still read inside the allocation's page.  A build that
should fail and does not is destroyed and failed; such a scene is never rendered.  No build is tried twice.

Not tested: the 2^28-entry limit of the grid list.  Its refused side needs a 1 GiB list on the host and the device (tens of seconds of
upload per case), its legal side 17 GB of pair records; both are left out.
"""
import copy
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch  # (before the library loads its HIP runtime: the order bench.py uses)

import oracle_lib
import prep_cases as PC
import prep_oracle as O
import scenarios
from conftest import golden_names, load_golden_scene
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu
THREADS = min(os.cpu_count() or 1, 16)
INT_MIN = -2 ** 31


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the scene upload tests cannot run (and the product has no CPU fallback)")
    t0 = time.time()
    yield
    print(f"\ntest_scene_prep_gpu.py: {time.time() - t0:.1f} s wall")


# ---- helpers ---------------------------------------------------------------------------------------------------------------------

def fetch(rs, names=("tri_rec", "tri_shade", "grid_bits", "block_sparse", "pair_rec", "cam_start", "cam_end", "cell_lut")):
    out = {n: rs.scene_view(n) for n in names}
    out["header"] = rs.scene_header()
    return out


def resident_arrays(sc, **kw):
    rs = R.ResidentScene(sc, **kw)
    try:
        return fetch(rs)
    finally:
        rs.close()


def device_view(arrays):
    return dict(words=arrays["grid_bits"], sparse=arrays["block_sparse"], pair_rec=arrays["pair_rec"])


def assert_dense_view(arrays, sc, what, decode_sample=None):
    """Words, sparse table and pair records equal the oracle's; the pair records' float words are the device's own triRec rows; the
    consumer's decode of the DEVICE arrays gives every non-empty cell's list and nothing for a sample of empty cells."""
    want = O.dense_view(sc.grid_start, sc.grid_list, O.triangle_records(sc.vertex, sc.tri_index, sc.tri_material, sc.tri_uv, sc.tri_normal)[0])
    got = device_view(arrays)
    assert arrays["header"]["pair_count"] == len(sc.grid_list) == len(got["pair_rec"]), what
    assert np.array_equal(got["words"], want["words"]), f"{what}: gridBits differs in {np.flatnonzero(got['words'] != want['words'])[:4]}"
    bad = np.flatnonzero(got["sparse"] != want["sparse"])
    assert bad.size == 0, f"{what}: gridBlockSparse differs in {bad.size} words, first {bad[:6]}: {got['sparse'][bad[:6]]} != {want['sparse'][bad[:6]]}"
    pr, wr = got["pair_rec"], want["pair_rec"]
    assert np.array_equal(pr[:, 3], wr[:, 3]), f"{what}: pair order differs at {np.flatnonzero(pr[:, 3] != wr[:, 3])[:6]}"
    assert np.array_equal(pr[:, 7], wr[:, 7]), f"{what}: pair count words differ at {np.flatnonzero(pr[:, 7] != wr[:, 7])[:6]}"
    own = O.pair_words(arrays["tri_rec"], pr[:, 3], pr[:, 7])
    assert np.array_equal(pr, own), f"{what}: pair records are not the device's triRec rows at {np.flatnonzero((pr != own).any(1))[:6]}"
    floats = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15]
    same = O.same_float_words(pr[:, floats].view(np.float32), wr[:, floats].view(np.float32))
    assert same.all(), f"{what}: pair records differ from the oracle's at {np.flatnonzero(~same.all(1))[:6]}"
    cells = np.flatnonzero(np.diff(sc.grid_start.astype(np.int64)))
    if decode_sample is not None and len(cells) > decode_sample:
        cells = np.random.default_rng(99).choice(cells, decode_sample, replace=False)
    bad = PC.decode_faults(got, sc.grid_start, sc.grid_list, cells, PC.empty_sample(sc.grid_start))
    assert bad == [], f"{what}: decode_cell on the device arrays is wrong for {len(bad)} cells, first {bad[:6]}"
    return len(cells)


def assert_triangle_records(arrays, sc, what):
    rec, shade = O.triangle_records(sc.vertex, sc.tri_index, sc.tri_material, sc.tri_uv, sc.tri_normal)
    assert arrays["header"]["triangle_count"] == sc.triangle_count
    for name, got, want in (("triRec", arrays["tri_rec"], rec), ("triShade", arrays["tri_shade"], shade)):
        assert got.shape == want.shape, (what, name)
        same = O.same_float_words(got, want)
        rows = np.flatnonzero(~same.all(1))
        assert rows.size == 0, (f"{what}: {name} differs in {rows.size} rows, first {rows[:4]}: got {got[rows[:2]].view(np.uint32)} "
                                f"want {want[rows[:2]].view(np.uint32)}")
    return rec


def assert_tile_major(arrays, sc, tiles, what):
    a, b, err = O.tile_major_ranges(sc.width, sc.height, tiles, sc.cam_start, sc.cam_end, len(sc.cam_list))
    assert err == 0, what
    assert arrays["header"]["tile_count"] == len(tiles) and arrays["header"]["tiles_x"] == (sc.width + 127) // 128
    for name, got, want in (("camStart", arrays["cam_start"], a), ("camEnd", arrays["cam_end"], b)):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0 and got.shape == want.shape, f"{what}: tile-major {name} differs in {bad.size} entries, first {bad[:6]}: {got[bad[:6]]} != {want[bad[:6]]}"


def assert_lut_and_tame(arrays, sc, what):
    planes = O.planes_of(sc.box_min)
    assert np.array_equal(arrays["cell_lut"].reshape(3, 256), O.cell_lut(planes)), f"{what}: cellLut"
    assert arrays["header"]["planes_tame"] == O.planes_tame(planes), f"{what}: planesTame"


def all_tiles(sc):
    return np.arange(R.tile_count(sc.width, sc.height), dtype=np.uint32)


def edit(sc, **arrays):
    out = copy.copy(sc)
    for k, v in arrays.items():
        setattr(out, k, np.ascontiguousarray(v))
    return out


def with_grid(sc, lists):
    start, glist = PC.grid_from_cells(lists)
    return edit(sc, grid_start=start, grid_list=glist)


def render(sc):
    return R.render_resident(sc)


def assert_renders_the_oracle_frame(sc, what):
    want = oracle_lib.oracle_render(sc, threads=THREADS)
    for name, got, exp in zip("RGB", render(sc), want):
        assert np.array_equal(got, exp.reshape(got.shape)), f"{what}: plane {name} differs from the oracle in {(got != exp.reshape(got.shape)).sum()} pixels"


def assert_refused(sc, mask, what, **kw):
    """The build fails with exactly the bits of `mask` in its text.  A scene that builds is destroyed at once and never used."""
    try:
        rs = R.ResidentScene(sc, **kw)
    except RuntimeError as e:
        assert str(e) == "rtHipSceneCreate failed: " + O.rejection_text(mask), what
        return
    rs.close()
    pytest.fail(f"{what}: the scene was built (wanted: {O.rejection_text(mask)})")


def assert_create_fails(desc, text, what, tiles=None, keep=()):
    """rtHipSceneCreate on a hand-edited description returns NULL with `text` in the error; `keep`: arrays the description points to."""
    ids = None if tiles is None else np.ascontiguousarray(tiles, np.uint32)
    h = R.lib().rtHipSceneCreate(0, C.byref(desc), None if ids is None else ids.ctypes.data, 0 if ids is None else len(ids))
    if h:
        R.lib().rtHipSceneDestroy(h)
        pytest.fail(f"{what}: the scene was built")
    assert text in R.last_error(), (what, R.last_error())


@pytest.fixture(scope="module")
def base():
    """A small textured scene with two materials and two lights, 200 x 150 (2 x 2 tiles), lists from the host builders."""
    mats = [dict(color=(200, 180, 90), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0)),
            dict(color=(40, 90, 220), reflection=(60, 60, 60), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(10, 0, 0))]
    lights = [dict(type=S.LIGHT_DISTANT, dir=(0.3, -0.8, 0.5), col=(1, 1, 1)), dict(type=S.LIGHT_OMNI, pos=(0.5, 1.0, 1.0), col=(0.4, 0.5, 0.3))]
    sc = S.make_soup(200, 150, 700, 0.25, seed=4242, samples=2, materials=mats, lights=lights, random_uv=True, name="prep_base")
    R.build_lists(sc)
    assert len(sc.cam_list) > 1000 and len(sc.grid_list) > 1000
    return sc


# ---- dense view, triangle records, ranges and tables on the golden scenes -------------------------------------------------------------

_golden = {}


def golden(name):
    if name not in _golden:
        sc, _ = load_golden_scene(name)
        _golden[name] = (sc, resident_arrays(sc))
    return _golden[name]


@pytest.mark.parametrize("name", golden_names())
def test_golden_triangle_records(name):
    sc, arrays = golden(name)
    assert_triangle_records(arrays, sc, name)


@pytest.mark.parametrize("name", golden_names())
def test_golden_dense_view(name):
    sc, arrays = golden(name)
    assert assert_dense_view(arrays, sc, name) > 0


@pytest.mark.parametrize("name", golden_names())
def test_golden_tile_major_ranges(name):
    sc, arrays = golden(name)
    assert_tile_major(arrays, sc, all_tiles(sc), name)


@pytest.mark.parametrize("name", golden_names())
def test_golden_cell_lut_and_planes_tame(name):
    sc, arrays = golden(name)
    assert_lut_and_tame(arrays, sc, name)


# ---- synthetic grids ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["counts", "last_block_empty", "random", "empty", "single"])
def test_synthetic_grid_dense_view(name, base):
    _golden.clear()
    lists = PC.synthetic_grids(base.triangle_count)[name]
    sc = with_grid(base, lists)
    arrays = resident_arrays(sc)
    assert assert_dense_view(arrays, sc, name) == len(lists)
    words = arrays["grid_bits"]
    if name == "counts":
        assert (words == np.uint64(0xFFFFFFFFFFFFFFFF)).sum() == 1 and words[-1] != 0 and words[0] & np.uint64(1)
    else:
        assert words[-1] == 0  # cellTotal is read from a last block that holds nothing
    if name == "empty":
        assert not words.any() and not arrays["block_sparse"].any() and arrays["pair_rec"].shape == (0, 16)


def test_million_triangle_soup():
    """The one large case; its decode check runs on a fixed sample of 100 000 non-empty cells, everything else on every element."""
    _golden.clear()
    sc = S.make_soup(256, 144, 1_000_000, 0.004, seed=12345, name="soup_1m")
    R.build_camera_list_device(sc)
    R.build_scene_grid_device(sc)
    arrays = resident_arrays(sc)
    assert_triangle_records(arrays, sc, "soup_1m")
    assert assert_dense_view(arrays, sc, "soup_1m", decode_sample=100_000) == 100_000
    assert_tile_major(arrays, sc, all_tiles(sc), "soup_1m")
    assert_lut_and_tame(arrays, sc, "soup_1m")


# ---- triangle records on awkward input -----------------------------------------------------------------------------------------------

def test_fuzz_triangle_records_with_degenerates_and_garbage():
    sc = scenarios.fuzz_scene(7)
    R.build_lists(sc)
    rng = np.random.default_rng(17)
    T = sc.triangle_count
    idx = sc.tri_index.copy()
    idx[:, 3] = rng.integers(INT_MIN, 2 ** 31, T)          # lane w is never read
    idx[0, 3], idx[1, 3], idx[2, 3] = -1, INT_MIN, sc.vertex_count
    idx[5, 1] = idx[5, 0]                                    # two corners alike: a line
    idx[6, 1] = idx[6, 2] = idx[6, 0]                        # a point: inv = 1 / 0
    vertex = sc.vertex.copy()
    vertex[idx[7, :3]] = [[1, 1, 1, 0], [2, 2, 2, 0], [3, 3, 3, 0]]  # collinear
    vertex[idx[8, 0], :3] = [3e38, -3e38, 3e38]                # overflowing differences: inf and NaN words
    vertex[idx[9, 0], :3] = [np.nan, 0, np.inf]
    vertex[idx[10, 0], :3] = [1e-40, -1e-42, 1e-45]            # subnormals
    vertex[:, 3] = rng.standard_normal(len(vertex))            # lane w of a vertex is never read
    mat = sc.tri_material.copy()
    mat[3], mat[4] = -1, INT_MIN
    ed = edit(sc, tri_index=idx, vertex=vertex, tri_material=mat)
    arrays = resident_arrays(ed)
    rec = assert_triangle_records(arrays, ed, "fuzz")
    assert np.isinf(rec[6, 15]) and np.isnan(rec[9]).any() and not np.isfinite(rec[8]).all()
    assert arrays["tri_shade"].view(np.uint32)[4, 21] == 0x80000000
    assert_dense_view(arrays, ed, "fuzz")  # the pair records carry the same inf / NaN words


# ---- tile-major ranges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (128, 128), (129, 1), (1, 257), (300, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_major_ranges_every_kind_of_range(size, base):
    _golden.clear()
    W, H = size
    sc = S.make_soup(W, H, 60, 0.3, seed=W + H, samples=1)
    R.build_lists(sc)
    rng = np.random.default_rng(1000 * W + H)
    P, L, T = W * H, 977, sc.triangle_count
    start = rng.integers(0, L + 1, P).astype(np.uint32)
    kind = rng.integers(0, 6, P)
    kind[:min(P, 6)] = np.arange(6)[:min(P, 6)]
    end = rng.integers(0, L + 1, P).astype(np.int64)                      # kind 0: anything legal, about half with end < start
    end[kind == 1] = start[kind == 1]                                     # end == start
    end[kind == 2] = L                                                    # end == list size
    end[kind == 3] = np.maximum(start[kind == 3].astype(np.int64) - 1, 0)  # end == start - 1
    start[kind == 4] = L                                                  # start == end == list size
    end[kind == 4] = L
    end[kind == 5] = np.minimum(start[kind == 5].astype(np.int64) + rng.integers(0, 3, int((kind == 5).sum())), L)
    end = end.astype(np.uint32)
    if P == 1:
        start[0], end[0] = L, L
    sc = edit(sc, cam_start=start, cam_end=end, cam_list=rng.integers(0, T, L).astype(np.uint32))
    assert (end < start).any() or P == 1
    assert_tile_major(resident_arrays(sc), sc, all_tiles(sc), f"{W}x{H} all tiles")
    tiles = rng.permutation(all_tiles(sc))[: max(1, (len(all_tiles(sc)) + 1) // 2)]
    if len(all_tiles(sc)) > 2:
        tiles = np.concatenate([tiles, tiles[:1]])  # a tile twice: two slots, the same ranges
    rs = R.ResidentScene(sc, tiles=tiles)
    try:
        assert_tile_major(fetch(rs, ("cam_start", "cam_end")), sc, tiles, f"{W}x{H} tiles {tiles}")
    finally:
        rs.close()


# ---- cellLut and planesTame ----------------------------------------------------------------------------------------------------------

def plane_sets():
    f = np.float32
    up, down = lambda v: np.nextafter(f(v), f(np.inf)), lambda v: np.nextafter(f(v), f(-np.inf))
    lo, hi = f(2.0 ** -60), f(2.0 ** 39)
    sets = {}
    for name, first, last, tame in (("at_2^-60", lo, 1.0, 1), ("below_2^-60", np.nextafter(lo, f(0)), 1.0, 0), ("at_-2^-60", -1.0, -lo, 1),
                                    ("above_-2^-60", -1.0, -np.nextafter(lo, f(0)), 0), ("at_2^39", 1.0, hi, 1), ("above_2^39", 1.0, up(hi), 0),
                                    ("at_-2^39", -hi, -1.0, 1), ("below_-2^39", down(-hi), -1.0, 0), ("zero_first", 0.0, 4.0, 1),
                                    ("minus_zero_last", -4.0, -0.0, 1)):
        p = np.tile(np.linspace(-1.0, 1.0, 257, dtype=np.float64).astype(f), (3, 1))
        p[1] = np.linspace(float(first), float(last), 257).astype(f)
        p[1, 0], p[1, 256] = first, last
        sets[name] = (p, tame)
    p = np.tile(np.linspace(-3.0, 5.0, 257).astype(f), (3, 1))
    p[0, 100] = p[0, 101]          # a repeated plane: a zero-width cell
    p[2, 1:200] = p[2, 0]          # two hundred of them
    p[1, 128] = -0.0
    sets["repeated"] = (p, 1)
    return sets


@pytest.mark.parametrize("name", sorted(plane_sets()))
def test_cell_lut_and_planes_tame_on_plane_sets(name, base):
    planes, tame = plane_sets()[name]
    assert O.planes_tame(planes) == tame
    box = np.zeros((257, 4), np.float32)
    box[:, :3] = planes.T
    sc = edit(base, box_min=box)
    rs = R.ResidentScene(sc)
    try:
        arrays = fetch(rs, ("cell_lut",))
    finally:
        rs.close()
    assert_lut_and_tame(arrays, sc, name)
    assert arrays["header"]["planes_tame"] == tame


def test_scene_view_refuses_bad_requests(base):
    rs = R.ResidentScene(base)
    try:
        L, out = R.lib(), np.zeros(64, np.uint32)
        n = L.rtHipTestSceneView(rs.handle, 3, 0, 0, None)
        assert n == base.triangle_count
        assert L.rtHipTestSceneView(rs.handle, 3, n, 0, out.ctypes.data) == 0
        for what, first, count, text in ((9, 0, 1, "unknown array"), (-1, 0, 1, "unknown array"), (3, n, 1, "reach past"), (3, 0, n + 1, "reach past"),
                                         (3, 2 ** 63, 2 ** 63, "reach past"), (0, 5, 1, "reach past"), (8, 768, 1, "reach past")):
            assert L.rtHipTestSceneView(rs.handle, what, first, count, out.ctypes.data) == -1 and text in R.last_error(), (what, first, count)
        assert not out.any()
        assert np.array_equal(rs.scene_view("tri_rec", n - 1, 1), rs.scene_view("tri_rec")[n - 1:])
    finally:
        rs.close()


# ---- refusals on the fresh build, and their legal neighbours -------------------------------------------------------------------------

def test_refuses_bad_vertex_ids_and_takes_the_last_vertex(base):
    V, T = base.vertex_count, base.triangle_count
    for lane, t in ((0, 0), (1, T // 2), (2, T - 1)):                   # nearest first: == V
        idx = base.tri_index.copy()
        idx[t, lane] = V
        assert_refused(edit(base, tri_index=idx), O.ERR_TRI_INDEX, f"vertex id == V in lane {lane} of triangle {t}")
    for far in (-1, INT_MIN):
        idx = base.tri_index.copy()
        idx[T // 3, 1] = far
        assert_refused(edit(base, tri_index=idx), O.ERR_TRI_INDEX, f"vertex id {far}")
    idx = base.tri_index.copy()
    idx[0, 0] = idx[T // 2, 1] = idx[T - 1, 2] = V - 1
    idx[:, 3] = [V, -1, INT_MIN, 2 ** 31 - 1] * (T // 4)                # lane w: any value
    assert_renders_the_oracle_frame(edit(base, tri_index=idx), "vertex id V - 1, garbage in lane w")


def test_refuses_bad_material_ids_and_takes_the_legal_ones(base):
    M, T = base.material_count, base.triangle_count
    assert M == 2
    for t in (0, T - 1):
        mat = base.tri_material.copy()
        mat[t] = M
        assert_refused(edit(base, tri_material=mat), O.ERR_TRI_MATERIAL, f"material == M on triangle {t}")
    none = S.make_soup(64, 48, 300, 0.2, seed=5, materials=[], name="no materials")
    R.build_lists(none)
    assert none.material_count == 0
    mat = none.tri_material.copy()
    mat[7] = 0
    assert_refused(edit(none, tri_material=mat), O.ERR_TRI_MATERIAL, "material 0 with no materials")
    mat = base.tri_material.copy()
    mat[T // 2] = 2 ** 31 - 1
    assert_refused(edit(base, tri_material=mat), O.ERR_TRI_MATERIAL, "material INT_MAX")
    mat = base.tri_material.copy()
    mat[0::3], mat[1::3], mat[2::3] = M - 1, -1, INT_MIN
    assert_renders_the_oracle_frame(edit(base, tri_material=mat), "materials M - 1, -1 and INT_MIN")
    assert_renders_the_oracle_frame(none, "no materials, every id -1")


def test_refuses_bad_camera_entries_and_takes_the_last_triangle(base):
    T, n = base.triangle_count, len(base.cam_list)
    for at in (0, n - 1, n // 2):
        cl = base.cam_list.copy()
        cl[at] = T
        assert_refused(edit(base, cam_list=cl), O.ERR_CAM_ENTRY, f"camera entry {at} == T")
    uncovered = np.concatenate([base.cam_list, [T]]).astype(np.uint32)  # an entry behind every pixel's range
    assert int(base.cam_end.max()) <= n
    assert_refused(edit(base, cam_list=uncovered), O.ERR_CAM_ENTRY, "camera entry == T that no range covers")
    cl = base.cam_list.copy()
    cl[n // 3] = 0xFFFFFFFF
    assert_refused(edit(base, cam_list=cl), O.ERR_CAM_ENTRY, "camera entry 0xffffffff")
    cl = base.cam_list.copy()
    cl[0] = cl[n // 2] = cl[n - 1] = T - 1
    assert_renders_the_oracle_frame(edit(base, cam_list=np.concatenate([cl, [T - 1]]).astype(np.uint32)), "camera entries T - 1")


def test_refuses_a_camera_range_past_the_list_and_takes_its_neighbours(base):
    n, W = len(base.cam_list), base.width
    inside_tile0, inside_tile3 = 10 * W + 10, 140 * W + 190
    end = base.cam_end.copy()
    end[inside_tile0] = n + 1
    bad = edit(base, cam_end=end)
    assert_refused(bad, O.ERR_CAM_RANGE, "range end == list size + 1")
    assert_refused(bad, O.ERR_CAM_RANGE, "the same on an instance that owns tile 0", tiles=[0, 2])
    end3 = base.cam_end.copy()
    end3[inside_tile3] = n + 1
    assert_refused(edit(base, cam_end=end3), O.ERR_CAM_RANGE, "range end == list size + 1 in the last tile")
    far = base.cam_end.copy()
    far[inside_tile0] = 0xFFFFFFFF
    assert_refused(edit(base, cam_end=far), O.ERR_CAM_RANGE, "range end 0xffffffff")
    # legal: end == list size (with start there too: an empty range at the very end), and end < start
    start, end = base.cam_start.copy(), base.cam_end.copy()
    start[inside_tile0], end[inside_tile0] = n, n
    end[inside_tile3] = n if start[inside_tile3] < n else end[inside_tile3]
    start[5 * W + 5], end[5 * W + 5] = base.cam_end[5 * W + 5], base.cam_start[5 * W + 5]
    grown = edit(base, cam_start=start, cam_end=end)
    assert_renders_the_oracle_frame(grown, "range end == list size, start == end == list size, end < start")
    # a range past the list in a tile this instance does not own is not read and therefore not refused (include/raytrace_hip.h,
    # rtHipSceneCreate): the instance renders its own tiles as if the range were sound
    want = oracle_lib.oracle_render(base, threads=THREADS)
    rs = R.ResidentScene(edit(base, cam_end=end3), tiles=[0, 1])
    try:
        rs.render()
        got = [p.reshape(base.height, base.width) for p in rs.readback()]
    finally:
        rs.close()
    for g, w in zip(got, want):
        assert np.array_equal(g[:128], w.reshape(g.shape)[:128]) and not g[128:].any()


def test_refuses_descending_grid_starts_and_takes_equal_ones(base):
    cells = O.CELLS
    assert base.grid_start[0] == base.grid_start[1] == 0
    gs = base.grid_start.copy()
    gs[0] = 1                                                   # start[0] > start[1]
    assert_refused(edit(base, grid_start=gs), O.ERR_GRID_MONOTONE, "start[0] > start[1]")
    gs = base.grid_start.copy()
    gs[cells] = gs[cells - 1] - 1                               # the last cell's start above the list's length
    assert_refused(edit(base, grid_start=gs), O.ERR_GRID_MONOTONE, "start[256^3 - 1] > start[256^3]")
    full = np.flatnonzero(np.diff(base.grid_start.astype(np.int64)))
    c = int(full[len(full) // 2])
    gs = base.grid_start.copy()
    gs[c] = gs[c + 1] + 1
    assert_refused(edit(base, grid_start=gs), O.ERR_GRID_MONOTONE, f"start[{c}] > start[{c + 1}]")
    gs = base.grid_start.copy()
    gs[c] = 0xFFFFFFFF
    assert_refused(edit(base, grid_start=gs), O.ERR_GRID_MONOTONE, "a start of 0xffffffff")
    assert (np.diff(base.grid_start.astype(np.int64)) == 0).sum() > cells // 2  # equal starts: most of the grid
    assert_renders_the_oracle_frame(base, "equal starts")


def test_refuses_bad_grid_entries_and_takes_the_last_triangle(base):
    T, n = base.triangle_count, len(base.grid_list)
    for at in (0, n - 1):
        gl = base.grid_list.copy()
        gl[at] = T
        assert_refused(edit(base, grid_list=gl), O.ERR_GRID_ENTRY, f"grid entry {at} == T")
    gl = base.grid_list.copy()
    gl[n // 2] = 0xFFFFFFFF
    assert_refused(edit(base, grid_list=gl), O.ERR_GRID_ENTRY, "grid entry 0xffffffff")
    gl = base.grid_list.copy()
    gl[0] = gl[n - 1] = T - 1
    assert_renders_the_oracle_frame(edit(base, grid_list=gl), "grid entries T - 1")


def test_two_faults_report_both_bits(base):
    """Faults of one part of the build are reported together.  (The build stops at the first part that fails -- geometry, then grid, then
    camera -- because the next part would gather through the bad ids: faults of different parts report the earlier part's bits.)"""
    T, V, M = base.triangle_count, base.vertex_count, base.material_count
    idx, mat = base.tri_index.copy(), base.tri_material.copy()
    idx[3, 2], mat[T - 2] = V, M
    assert_refused(edit(base, tri_index=idx, tri_material=mat), O.ERR_TRI_INDEX | O.ERR_TRI_MATERIAL, "vertex and material")
    cl, end = base.cam_list.copy(), base.cam_end.copy()
    cl[1], end[20 * base.width + 20] = T, len(cl) + 1
    assert_refused(edit(base, cam_list=cl, cam_end=end), O.ERR_CAM_ENTRY | O.ERR_CAM_RANGE, "camera entry and range")
    gs, gl = base.grid_start.copy(), base.grid_list.copy()
    gs[0], gl[len(gl) - 1] = 1, T
    assert_refused(edit(base, grid_start=gs, grid_list=gl), O.ERR_GRID_MONOTONE | O.ERR_GRID_ENTRY, "grid starts and entry")
    assert_refused(edit(base, tri_index=idx, grid_list=gl, cam_list=cl), O.ERR_TRI_INDEX, "geometry fails first")
    assert_refused(edit(base, grid_list=gl, cam_list=cl), O.ERR_GRID_ENTRY, "then the grid")


# ---- the same refusals on the clone route, the cached update and with device arrays ---------------------------------------------------

def test_a_like_clone_with_a_bad_camera_list_is_refused(base):
    T, n = base.triangle_count, len(base.cam_list)
    root = R.ResidentScene(base, tiles=[0, 3])
    try:
        cl = base.cam_list.copy()
        cl[n - 1] = T
        assert_refused(edit(base, cam_list=cl), O.ERR_CAM_ENTRY, "clone: camera entry == T", tiles=[1, 2], like=root)
        end = base.cam_end.copy()
        end[10 * base.width + 150] = n + 1  # tile 1
        assert_refused(edit(base, cam_end=end), O.ERR_CAM_RANGE, "clone: range end == list size + 1", tiles=[1, 2], like=root)
        cl[n - 1] = 0xFFFFFFFF
        assert_refused(edit(base, cam_list=cl), O.ERR_CAM_ENTRY, "clone: camera entry 0xffffffff", tiles=[1, 2], like=root)
        cl[n - 1] = T - 1
        legal = edit(base, cam_list=cl)
        want = [p.reshape(base.height, base.width) for p in oracle_lib.oracle_render(legal, threads=THREADS)]
        peer = R.ResidentScene(legal, tiles=[1, 2], like=root)
        try:
            assert fetch(peer, ())["header"]["pair_count"] == len(base.grid_list)
            assert_dense_view(fetch(peer), legal, "clone")  # the copied grid part is the root's, array for array
            peer.render()
            got = [p.reshape(base.height, base.width) for p in peer.readback()]
        finally:
            peer.close()
        root.render()  # the refused clones left the root whole
        mine = [p.reshape(base.height, base.width) for p in root.readback()]
        base_want = [p.reshape(base.height, base.width) for p in oracle_lib.oracle_render(base, threads=THREADS)]
        for g, m, w, bw in zip(got, mine, want, base_want):
            assert np.array_equal(g[:128, 128:], w[:128, 128:]) and np.array_equal(g[128:, :128], w[128:, :128])
            assert np.array_equal(m[:128, :128], bw[:128, :128]) and np.array_equal(m[128:, 128:], bw[128:, 128:])
    finally:
        root.close()


def cache_is_empty():
    return R.lib().rtHipTestCachePointers((C.c_void_p * 6)()) == -2


def test_the_cached_update_refuses_and_forgets(base):
    T = base.triangle_count
    want = oracle_lib.oracle_render(base, threads=THREADS)

    def warm(what):
        ok, r, g, b = R.raytrace_all(1, base)
        assert ok, R.last_error()
        for got, exp in zip((r, g, b), want):
            assert np.array_equal(got, exp.reshape(got.shape)), what
        assert not cache_is_empty()

    R.lib().rtHipCacheClear()
    try:
        warm("first call")
        # (a) a camera-only edit brings a bad entry in
        cl = base.cam_list.copy()
        cl[len(cl) // 2] = T
        ok, r, g, b = R.raytrace_all(1, edit(base, cam_list=cl))
        assert not ok and R.last_error() == O.rejection_text(O.ERR_CAM_ENTRY) and cache_is_empty()
        warm("after the refused camera edit")
        # (b) a geometry edit takes the last triangle away under an unchanged camera list (the grid is the smaller scene's own): an old
        # camera entry is now == T
        assert (base.cam_list == T - 1).any()
        less = edit(base, tri_index=base.tri_index[:T - 1], tri_material=base.tri_material[:T - 1], tri_uv=base.tri_uv[:3 * (T - 1)],
                    tri_normal=base.tri_normal[:3 * (T - 1)])
        R.build_scene_grid(less)
        assert int(less.grid_list.max()) < T - 1
        ok, r, g, b = R.raytrace_all(1, less)
        assert not ok and R.last_error() == O.rejection_text(O.ERR_CAM_ENTRY) and cache_is_empty()
        warm("after the refused geometry edit")
        # a camera range past the list, and a grid fault, through the same route
        end = base.cam_end.copy()
        end[0] = len(base.cam_list) + 1
        ok, r, g, b = R.raytrace_all(1, edit(base, cam_end=end))
        assert not ok and R.last_error() == O.rejection_text(O.ERR_CAM_RANGE) and cache_is_empty()
        warm("after the refused camera range")
        gl = base.grid_list.copy()
        gl[0] = T
        ok, r, g, b = R.raytrace_all(1, edit(base, grid_list=gl))
        assert not ok and R.last_error() == O.rejection_text(O.ERR_GRID_ENTRY) and cache_is_empty()
        warm("after the refused grid edit")
    finally:
        R.lib().rtHipCacheClear()


def on_device(sc):
    out = copy.copy(sc)
    for k, v in vars(sc).items():
        if isinstance(v, np.ndarray):
            a = np.ascontiguousarray(v)
            a = a.view(np.int32) if a.dtype == np.uint32 else a
            setattr(out, k, torch.from_numpy(a.copy()).cuda())
    return out


def test_refusals_with_device_arrays(base):
    T, V = base.triangle_count, base.vertex_count
    gl = base.grid_list.copy()
    gl[len(gl) - 1] = T
    assert_refused(on_device(edit(base, grid_list=gl)), O.ERR_GRID_ENTRY, "device arrays: last grid entry == T")
    gs = base.grid_start.copy()
    gs[O.CELLS] = gs[O.CELLS - 1] - 1  # the list size the library fetches from the device is the descending one
    assert_refused(on_device(edit(base, grid_start=gs)), O.ERR_GRID_MONOTONE, "device arrays: last start descends")
    cl = base.cam_list.copy()
    cl[0] = T
    assert_refused(on_device(edit(base, cam_list=cl)), O.ERR_CAM_ENTRY, "device arrays: camera entry == T")
    idx = base.tri_index.copy()
    idx[T - 1, 2] = V
    assert_refused(on_device(edit(base, tri_index=idx)), O.ERR_TRI_INDEX, "device arrays: vertex id == V")
    dev = on_device(base)
    rs = R.ResidentScene(dev)
    try:
        arrays = fetch(rs)
        rs.render()
        got = rs.readback()
    finally:
        rs.close()
    assert_dense_view(arrays, base, "device arrays")
    assert_triangle_records(arrays, base, "device arrays")
    for g, w in zip(got, oracle_lib.oracle_render(base, threads=THREADS)):
        assert np.array_equal(g.reshape(w.shape), w)


# ---- host-side refusals of the build ---------------------------------------------------------------------------------------------------

def test_host_side_refusals(base):
    def desc(**fields):
        d = R.scene_desc(base)
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    assert_create_fails(desc(width=0), "empty image", "zero width")
    assert_create_fails(desc(height=0), "empty image", "zero height")
    assert_create_fails(desc(sampleCount=0), "sampleCount", "no samples")
    for div in (255, 257, 0, -256):
        assert_create_fails(desc(axesDiv=div), "axesDivCount", f"axesDiv {div}")
    for field in ("camStart", "camEnd", "camList", "vertex", "triIndex", "triMaterial", "triUv", "triNormal", "boxMin", "gridStart", "gridList",
                  "matSize", "matStart", "textures", "lightType", "lightPos", "lightDir", "lightCol", "lightRadius", "lightHalfAtt"):
        assert_create_fails(desc(**{field: None}), "null", f"null {field}")
    tiles = R.tile_count(base.width, base.height)
    assert_create_fails(desc(), "tile id", "tile id == tile count", tiles=[0, tiles])
    assert_create_fails(desc(), "tile id", "tile id 0xffffffff", tiles=[0xFFFFFFFF])


def test_material_channels_at_the_end_of_the_atlas():
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (4, 4, 3)).astype(np.uint8)
    mats = [dict(color=(255, 255, 255), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=img)]
    sc = S.make_soup(64, 48, 300, 0.3, seed=12, samples=1, materials=mats, random_uv=True)
    R.build_lists(sc)
    texels = len(sc.textures)
    assert sc.mat_start[4] + 16 == texels  # the image ends exactly at the atlas
    assert_renders_the_oracle_frame(sc, "an image that ends exactly at the atlas")
    for what, channel, value in (("one texel past the atlas", 4, sc.mat_start[4] + 1), ("a negative start", 4, -1), ("a negative start of a texel", 0, -1),
                                 ("a start of INT_MIN", 4, INT_MIN)):
        ms = sc.mat_start.copy()
        ms[channel] = value
        ed = edit(sc, mat_start=ms)
        assert_create_fails(R.scene_desc(ed), "exceed the", what, keep=(ed,))


def test_light_count_limit():
    def many(n):
        sc = S.make_soup(8, 8, 20, 0.3, seed=2, samples=1)
        R.build_lists(sc)
        sc.light_type = np.full(n, S.LIGHT_DISTANT, np.int32)
        for k in ("light_pos", "light_dir", "light_col"):
            setattr(sc, k, np.tile(np.array([[0.3, -0.8, 0.5, 0.0]], np.float32), (n, 1)))
        sc.light_radius, sc.light_half_att = np.full(n, 0.5, np.float32), np.full(n, np.inf, np.float32)
        return sc

    sc = many(65536)
    assert_create_fails(R.scene_desc(sc), "lightCount 65536 too large", "65536 lights", keep=(sc,))
    rs = R.ResidentScene(many(65535))
    rs.close()
