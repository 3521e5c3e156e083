"""The scene-upload oracle (prep_oracle.py) checked on the CPU before it judges the device (test_scene_prep_gpu.py):
dense_view and decode_cell against a plain Python loop over the non-empty cells of small synthetic grids, the comparers against six
host-made corruptions of a correct view (each must be caught), tile_major_ranges / triangle_records / cell_lut / planes_tame on
hand-checked cases, and the refusals of rtHipTestSceneView that need no device.

Every scene-building entry point asks for a HIP device before it looks at its description (scene_create, RaytraceAll), so none of
scene_build's host-side refusals can be reached without a GPU: they are all in test_scene_prep_gpu.py."""
import numpy as np
import pytest

import prep_cases as PC
import prep_oracle as O
from opencl_render_amd import raytrace as R

T = 400


@pytest.fixture(scope="module")
def tri_rec():
    rng = np.random.default_rng(3)
    return rng.standard_normal((T, 16)).astype(np.float32)


@pytest.fixture(scope="module")
def grids():
    return PC.synthetic_grids(T)


@pytest.fixture(scope="module")
def views(grids, tri_rec):
    out = {}
    for name, lists in grids.items():
        start, glist = PC.grid_from_cells(lists)
        out[name] = (start, glist, O.dense_view(start, glist, tri_rec))
    return out


def loop_view(lists, tri_rec):
    """The dense view by a plain loop over the non-empty cells, straight from the RtDevScene comment."""
    bits = np.asarray(tri_rec, np.float32).view(np.uint32)
    order = sorted(lists, key=lambda c: (((c & 255) >> 2) + 64 * (((c >> 8) & 255) >> 2) + 4096 * ((c >> 16) >> 2),
                                         (c & 3) | ((c >> 8) & 3) << 2 | ((c >> 16) & 3) << 4))
    words, first_of_block = {}, {}
    for k, c in enumerate(order):
        cx, cy, cz = O.cell_xyz(c)
        block = (cx >> 2) + 64 * (cy >> 2) + 4096 * (cz >> 2)
        words[block] = words.get(block, 0) | 1 << ((cx & 3) | (cy & 3) << 2 | (cz & 3) << 4)
        first_of_block.setdefault(block, k)
    pairs = sum(len(v) for v in lists.values())
    tri, info = [0] * pairs, [0] * pairs
    rest = len(order)
    for k, c in enumerate(order):
        ids = lists[c]
        tri[k], info[k] = ids[0], min(len(ids), 15) | rest << 4
        for i in range(1, len(ids)):
            tri[rest], info[rest] = ids[i], len(ids) if i == 1 else 0
            rest += 1
    rec = np.zeros((pairs, 16), np.uint32)
    for p in range(pairs):
        r = bits[tri[p]]
        rec[p] = [r[0], r[1], r[2], tri[p], r[9], r[10], r[11], info[p], r[3], r[4], r[5], r[13], r[6], r[7], r[8], r[15]]
    return words, first_of_block, rec, len(order)


@pytest.mark.parametrize("name", ["counts", "last_block_empty", "random", "empty", "single"])
def test_dense_view_equals_the_plain_loop(name, grids, views, tri_rec):
    lists = grids[name]
    start, glist, view = views[name]
    words, first_of_block, rec, cells = loop_view(lists, tri_rec)
    assert view["cells"] == cells
    assert np.array_equal(view["pair_rec"], rec)
    want_words = np.zeros(O.BLOCKS, np.uint64)
    for b, w in words.items():
        want_words[b] = w
    assert np.array_equal(view["words"], want_words)
    # the sparse table: every block's entry {lo, hi, rank}, rank = non-empty cells of all blocks before it; every other slot zero
    want = np.zeros(O.SPARSE_WORDS, np.uint32)
    per_block = np.zeros(O.BLOCKS, np.int64)
    for b, w in words.items():
        per_block[b] = bin(w).count("1")
    rank = np.cumsum(per_block) - per_block
    for b in range(O.BLOCKS):
        if rank[b] == 0 and b not in words:
            continue  # (all three words zero)
        e = 3 * ((b & 63) | ((b >> 6) & 63) << 8 | (b >> 12) << 16)
        w = words.get(b, 0)
        want[e:e + 3] = (w & 0xFFFFFFFF, w >> 32, rank[b])
    assert np.array_equal(view["sparse"], want)
    for b, k in first_of_block.items():
        assert rank[b] == k


@pytest.mark.parametrize("name", ["counts", "last_block_empty", "random", "empty", "single"])
def test_decode_cell_returns_every_cells_list(name, grids, views):
    lists = grids[name]
    start, glist, view = views[name]
    for c, ids in lists.items():
        assert O.decode_cell(view, *O.cell_xyz(c)) == ids, c
    empties = PC.empty_sample(start)
    assert len(empties) > 2000
    assert PC.decode_faults(view, start, glist, lists.keys(), empties) == []


def test_the_counts_grid_holds_what_it_promises(grids, views):
    lists = grids["counts"]
    sizes = {len(v) for v in lists.values()}
    assert {1, 2, 14, 15, 16, 300} <= sizes
    start, glist, view = views["counts"]
    words = view["words"]
    assert (words == np.uint64(0xFFFFFFFFFFFFFFFF)).sum() == 1 and (words == np.uint64(1)).sum() >= 1 and (words == np.uint64(1 << 63)).sum() >= 2
    for c in PC.CORNERS:
        assert PC.cell_id(*c) in lists
    assert words[O.BLOCKS - 1] != 0 and views["last_block_empty"][2]["words"][O.BLOCKS - 1] == 0 and views["random"][2]["words"][O.BLOCKS - 1] == 0
    assert max(np.bincount(glist)) >= 90  # one triangle in many cells
    assert len(views["empty"][1]) == 0 and len(views["single"][1]) == 1


# ---- the checks bite: six corruptions of a correct view, each caught ------------------------------------------------------------

def copy_view(view):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in view.items()}


def dense_id(view, c):
    cx, cy, cz = O.cell_xyz(c)
    e = 3 * ((cx >> 2) | (cy >> 2) << 8 | (cz >> 2) << 16)
    word = int(view["sparse"][e]) | int(view["sparse"][e + 1]) << 32
    bit = (cx & 3) | (cy & 3) << 2 | (cz & 3) << 4
    return int(view["sparse"][e + 2]) + bin(word & ((1 << bit) - 1)).count("1")


def cell_with(lists, n):
    return next(c for c in sorted(lists) if len(lists[c]) == n)


def swap_y_z_bits(view):
    """The view a producer with bit order x | z<<2 | y<<4 would write (words and block table; pair order left alone)."""
    w = view["words"]
    out = np.zeros_like(w)
    for bit in range(64):
        x, y, z = bit & 3, (bit >> 2) & 3, bit >> 4
        out |= ((w >> np.uint64(bit)) & np.uint64(1)) << np.uint64(x | z << 2 | y << 4)
    view["words"] = out
    b = np.arange(O.BLOCKS, dtype=np.int64)
    at = 3 * ((b & 63) | ((b >> 6) & 63) << 8 | (b >> 12) << 16)
    view["sparse"][at] = (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    view["sparse"][at + 1] = (out >> np.uint64(32)).astype(np.uint32)


def corruptions(lists, view):
    """name -> (corrupt(view), caught by the array comparison, caught by the decode)."""
    def rest_off_by_one(v):
        v["pair_rec"][dense_id(v, cell_with(lists, 2)), 7] += 16

    def fifteen_for_fourteen(v):
        k = dense_id(v, cell_with(lists, 14))
        assert v["pair_rec"][k, 7] & 15 == 14
        v["pair_rec"][k, 7] |= 15

    def count_on_second_further(v):
        k = dense_id(v, cell_with(lists, 16))
        rest = int(v["pair_rec"][k, 7]) >> 4
        assert v["pair_rec"][rest, 7] == 16 and v["pair_rec"][rest + 1, 7] == 0
        v["pair_rec"][rest, 7], v["pair_rec"][rest + 1, 7] = 0, 16

    def unused_sparse_slot(v):
        slot = 3 * (64 | 5 << 8 | 9 << 16)  # bx = 64 does not exist
        assert v["sparse"][slot + 1] == 0
        v["sparse"][slot + 1] = 1

    def pair_triangle_changed(v):
        rest = int(v["pair_rec"][dense_id(v, cell_with(lists, 300)), 7]) >> 4
        v["pair_rec"][rest + 100, 3] ^= 1

    # 15 for 14 decodes to the same list (the first further record carries the exact count of every cell that has one), and nothing
    # reads an unused slot: those two are caught by the array comparison alone, which is why the GPU tests always run both checks
    return {"y_z_swapped": (swap_y_z_bits, True, True), "rest_off_by_one": (rest_off_by_one, True, True),
            "fifteen_for_fourteen": (fifteen_for_fourteen, True, False), "count_on_second_further": (count_on_second_further, True, True),
            "unused_sparse_slot": (unused_sparse_slot, True, False), "pair_triangle_changed": (pair_triangle_changed, True, True)}


@pytest.mark.parametrize("which", ["y_z_swapped", "rest_off_by_one", "fifteen_for_fourteen", "count_on_second_further", "unused_sparse_slot",
                                   "pair_triangle_changed"])
def test_every_corruption_of_a_correct_view_is_caught(which, grids, views):
    lists = grids["counts"]
    start, glist, good = views["counts"]
    assert PC.compare_views(good, good) == [] and PC.decode_faults(good, start, glist, lists.keys()) == []
    corrupt, by_compare, by_decode = corruptions(lists, good)[which]
    bad = copy_view(good)
    corrupt(bad)
    assert bool(PC.compare_views(bad, good)) == by_compare
    assert bool(PC.decode_faults(bad, start, glist, lists.keys(), PC.empty_sample(start))) == by_decode
    assert by_compare or by_decode


# ---- the other restatements on cases worked by hand -----------------------------------------------------------------------------

def test_tile_major_ranges_by_hand():
    W, H = 130, 3  # two tiles in a row; the second holds two columns
    P = W * H
    start = np.arange(P, dtype=np.uint32)
    end = start + 2
    end[5] = 1          # end < start: empty at start
    end[W + 129] = P + 2  # == list size: legal
    a, b, err = O.tile_major_ranges(W, H, [1, 0], start, end, P + 2)
    assert err == 0 and a.shape == (2 * O.TILE_PIXELS,)
    assert (a[0], b[0]) == (128, 130) and (a[1], b[1]) == (129, 131) and (a[2], b[2]) == (0, 0)  # tile 1: columns 128, 129, then overhang
    assert (a[128 + 1], b[128 + 1]) == (W + 129, P + 2)
    assert (a[3 * 128], b[3 * 128]) == (0, 0)  # row 3 does not exist
    t0 = O.TILE_PIXELS
    assert (a[t0 + 5], b[t0 + 5]) == (5, 5) and (a[t0 + 2 * 128 + 127], b[t0 + 2 * 128 + 127]) == (2 * W + 127, 2 * W + 129)
    assert np.count_nonzero(b) == P and np.count_nonzero(b[:t0]) == 6  # every pixel once, nothing in the overhang
    end[7] = P + 3      # one past the list
    a, b, err = O.tile_major_ranges(W, H, [0], start, end, P + 2)
    assert err == O.ERR_CAM_RANGE and (a[7], b[7]) == (0, 0) and (a[8], b[8]) == (8, 10)
    a, b, err = O.tile_major_ranges(W, H, [1], start, end, P + 2)  # the bad pixel is in tile 0: tile 1 alone does not see it
    assert err == 0


def test_triangle_records_by_hand():
    vertex = np.array([[1, 2, 3, 99], [2, 2, 3, 99], [1, 4, 3, 99], [5, 5, 5, 0]], np.float32)
    idx = np.array([[0, 1, 2, 12345], [3, 3, 3, -7]], np.int32)
    mat = np.array([-1, -2 ** 31], np.int32)
    uv = np.arange(12, dtype=np.float32).reshape(6, 2)
    nrm = np.arange(24, dtype=np.float32).reshape(6, 4)
    rec, shade = O.triangle_records(vertex, idx, mat, uv, nrm)
    # ab = (1,0,0), ac = (0,2,0), n = cross(ac, ab) = (0,0,-2), abab 1, abac 0, acac 4, inv = 1 / (0 - 4)
    assert list(rec[0]) == [1, 2, 3, 1, 0, 0, 0, 2, 0, 0, 0, -2, 1, 0, 4, -0.25]
    assert list(rec[1][:15]) == [5, 5, 5] + [0] * 12 and np.isinf(rec[1][15])  # a point: 1 / 0
    assert list(shade[0][:6]) == [2, 2, 3, 1, 4, 3] and list(shade[0][6:15]) == [0, 1, 2, 4, 5, 6, 8, 9, 10] and list(shade[0][15:21]) == [0, 1, 2, 3, 4, 5]
    assert shade.view(np.uint32)[0, 21] == 0xFFFFFFFF and shade.view(np.uint32)[1, 21] == 0x80000000
    assert not shade[:, 22:].any()
    nan = np.array([np.nan, 1.0], np.float32)
    assert O.same_float_words(nan, np.array([-np.nan, 1.0], np.float32)).all() and not O.same_float_words(nan, np.array([1.0, 1.0], np.float32))[0]
    assert not O.same_float_words(np.array([0.0], np.float32), np.array([-0.0], np.float32))[0]


def test_cell_lut_and_planes_tame_by_hand():
    planes = np.tile(np.arange(257, dtype=np.float32), (3, 1))  # unit cells over 0..256: step i's middle i + 0.5 lies in cell i
    assert np.array_equal(O.cell_lut(planes), np.tile(np.arange(256, dtype=np.uint8), (3, 1)))
    planes[1, 1:256] = 256.0  # all inner planes at the far end: every middle is still in cell 0
    planes[2, 1:256] = 0.0    # all inner planes at the near end: every middle is in the last cell
    lut = O.cell_lut(planes)
    assert not lut[1].any() and (lut[2] == 255).all()
    assert O.planes_tame(planes) == 1
    for v, tame in ((2.0 ** -60, 1), (-2.0 ** -60, 1), (2.0 ** 39, 1), (-2.0 ** 39, 1), (0.0, 1), (-0.0, 1),
                    (np.nextafter(np.float32(2.0 ** -60), np.float32(0)), 0), (np.nextafter(np.float32(2.0 ** 39), np.float32(np.inf)), 0),
                    (-np.nextafter(np.float32(2.0 ** 39), np.float32(np.inf)), 0), (np.inf, 0), (np.nan, 0)):
        p = planes.copy()
        p[0, 100] = v
        assert O.planes_tame(p) == tame, v


def test_rejection_text():
    assert O.rejection_text(4) == "scene rejected (0x4): a camera list entry is not a triangle;"
    assert O.rejection_text(3) == "scene rejected (0x3): a triangle references a vertex that does not exist; a triangle uses a material >= materialCount;"


# ---- rtHipTestSceneView: what it refuses without a device -----------------------------------------------------------------------

def test_scene_view_refuses_a_null_scene(hip_lib):
    out = np.zeros(8, np.uint32)
    for what in (0, 3, 99, -1):
        assert hip_lib.rtHipTestSceneView(None, what, 0, 1, out.ctypes.data) == -1
        assert "null scene" in R.last_error()
        assert hip_lib.rtHipTestSceneView(None, what, 0, 0, None) == -1
    assert not out.any()
    assert sorted(v[0] for v in R.SCENE_VIEWS.values()) == list(range(9))
